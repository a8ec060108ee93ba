"""Parity of ``ssi_decode_sample`` (csrc/decode_sample.hip): the float64 sampler of ``include/ssi_hip.h``, the three bounds derived from the
kernel's rounding points, an fp32 restatement of the kernel with its mutants for the checker's CPU self-test, and the inputs that
tests/test_decode_sample_ref.py (CPU) and tests/test_decode_sample_gpu.py (GPU) share.  Philox is tests/sr_ref.py's; the logits families,
masks and pads are tests/decode_select_ref.py's.

The definition, per row on the STORED values (upcast to float64), with the mask the row takes:
  A      the allowed columns below vocab; values ordered with NaN below every number (``order_key``);
  K      {c in A: x_c >= the top_k-th largest of A} when 0 < top_k < |A| (ties at the threshold stay), else A;
  P      {c in K: x_c >= tp}: tp the largest value v of K with M(v) >= top_p Z, w_c = exp((x_c - max_K x) / T), Z = sum_K w,
         M(v) = sum of w over {c in K: x_c >= v}; K when top_p >= 1;
  token  argmax over P of x_c / T + G_c, the lowest column on a tie; G_c = -ln(-ln u_c), u_c = (2 (w_c >> 9) + 1) 2^-24, w_c word c & 3 of
         Philox4x32-10 at counter (c >> 2, step, sequence, 0x53414D50), key (seed lo, seed hi);
         when no column of A holds a number above -inf: the first allowed column, and P is that column; nothing allowed: -1 / 0 / -1;
  logprob = x[token] - logsumexp(x[:vocab]) (T = 1, all real columns); n_kept = |P|.

The bounds (DERIVED from the kernel's rounding points, not measured; U32 = 2^-24 is half an fp32 ulp, relatively):

logprob: ``decode_select_ref.Base.dlse`` + U32 |logprob| — the kernel's exp-sum is ssi_decode_select's, term for term.

Score bound delta_c of fma(x_c, fl(1 / T), G_c) against x_c / T + G_c:  fl(1 / T) is off by U32 relatively: U32 |x_c| / T.  The inner
logarithm l = -ln u is logf(u) for u < 1/2 (|ln u| >= ln 2: logf's relative 2 ACC_LOGF U32) and log1pf(u - 1) above, on the EXACT u - 1
(log1pf's documented accuracy is logf's; the same 2 ACC_LOGF U32 is taken).  The outer logf sees that relative error as an absolute one of
its result, 2 ACC_LOGF U32, and adds its own 2 ACC_LOGF U32 max(|G|, 1) (relative where |G| >= 1, and no worse than that absolutely around
l = 1 where G passes 0).  The fma rounds once: U32 |score|.  Together
    delta_c = U32 (|x_c| / T + |score_c|) + 2 ACC_LOGF U32 (1 + max(|G_c|, 1)).
A row is judged when the reference's best and second-best scores in P differ by more than 2 max_c delta_c.

Mass bound eps of M(v) / Z:  a term is exp2(fma(x, sc, nm)), sc = fl(log2 e / T), nm = fl(-m sc).  x sc + nm = (x - m) sc + (m sc + nm): the
second part is the same for every column of the row, a common factor of all masses that leaves M / Z alone.  (x - m) sc is off by
U32 (m - x) log2 e / T (sc rounded) and the fma's rounding adds U32 |argument| = the same again: relatively 2 U32 (m - x) / T on the term,
plus v_exp_f32's 2 ACC_V_EXP U32.  The term times 2^40 is truncated to an integer: 2^-40 absolutely, of a Z that is at least 1 (the maximum's
term).  Integer sums are exact.  M >= ceil(top_p Z) in integers with the product in fp64: one unit and 2^-52 relatively.  With
e = sum_K w_c rel_c + |K| 2^-40 (all over the exact Z), both M and Z are off by at most e, so M / Z by at most 2 e:
    eps = 2 (sum_K w_c (2 U32 (m - x_c) / T + 2 ACC_V_EXP U32) / Z + |K| 2^-40) + 2^-39.
A row with a class at |M(v) - top_p Z| / Z <= eps is AMBIGUOUS: n_kept may be either neighbour and the token is the reference's draw from
the set the kernel reported."""
import functools
import math

import numpy as np
import torch

import decode_select_ref as D
import sr_ref
from ce_parity import ACC_LOGF, ACC_V_EXP, BF16, F32, LOG2E, U32

TAG = 0x53414D50
VOCABS = (1, 7, 8, 9, 255, 257, 2049, D.FLAGSHIP[0])
ROWS = (1, 3, 257)
TEMPS = (0.7, 1.0, 1.3)
TOP_PS = (1.0, 0.9, 0.5, 1e-6)
MUTANTS = ("mask_ignored", "mask_in_lse", "topp_before_topk", "ties_dropped", "temp_in_logprob", "sequence_ignored", "u32")
MAX_AMBIGUOUS_FLAGSHIP = 0.25


def top_ks(vocab):
    return (-1, 1, 2, 50, vocab, vocab + 1)


def settings(vocab):
    """Every (top_k, top_p) pair, the temperatures and the mask kinds that exist at this vocabulary taken in turn."""
    kinds = [k for k in D.MASK_KINDS if D.mask_exists(k, vocab)]
    out = []
    for i, k in enumerate(top_ks(vocab)):
        for j, p in enumerate(TOP_PS):
            n = i * len(TOP_PS) + j
            out.append(dict(T=TEMPS[n % 3], top_k=k, top_p=p, kind=kinds[n % len(kinds)]))
    return out


# ---- the random bits and the Gumbel values ---------------------------------------------------------------------------------------------
def philox_words(seqs, vocab, seed, step):
    """int64 [rows, vocab]: word c & 3 of Philox4x32-10 at counter (c >> 2, step, sequence, TAG) under key (seed lo, seed hi)."""
    seqs = torch.as_tensor(seqs, dtype=torch.int64).reshape(-1) & sr_ref.M32
    nb = (vocab + 3) // 4
    blk = torch.arange(nb, dtype=torch.int64)[None, :].expand(seqs.numel(), nb)
    w = sr_ref.philox4x32_10((blk, int(step), seqs[:, None].expand(-1, nb), TAG), (seed & sr_ref.M32, (seed >> 32) & sr_ref.M32))
    return torch.stack(w, dim=-1).reshape(seqs.numel(), nb * 4)[:, :vocab].numpy()


def gumbel64(words):
    u = (2 * (words >> 9) + 1).astype(np.float64) * 2.0 ** -24
    return -np.log(-np.log(u))


def order_key(x):
    """float64 keys whose order is the kernel's: NaN below -inf below every number (-0 equals +0 already)."""
    k = x.copy()
    k[np.isneginf(x)] = -1e300
    k[np.isnan(x)] = -np.inf
    return k


def _first_best(cols, score):
    """The column of ``cols`` with the largest score, the lowest on a tie; a NaN score is never taken."""
    s = np.where(np.isnan(score), -np.inf, score)
    best = s.max()
    return int(cols[s == best].min())


class Expected:
    def __init__(self, rows):
        self.token = np.full(rows, -1, dtype=np.int64)
        self.n_kept = np.full(rows, -1, dtype=np.int64)
        self.margin_ok = np.ones(rows, dtype=bool)
        self.gap = np.full(rows, math.inf)                 # best - second-best score in P
        self.ambiguous = np.zeros(rows, dtype=bool)
        self.alts = [dict() for _ in range(rows)]          # for an ambiguous row: {n_kept: token} of every set the kernel may report
        self.worst_margin = math.inf                       # min over rows of (best - second) / (2 max delta)
        self.worst_mass = math.inf                         # min over rows and classes of |M / Z - top_p| / eps


class Case:
    """One [rows, ld] input with its sequences, seed and step: what every setting of the sampler shares."""

    def __init__(self, x, vocab, seqs, seed, step, vec=None):
        self.x, self.vocab, self.seed, self.step = x, vocab, int(seed), int(step)
        self.seqs = torch.as_tensor(seqs, dtype=torch.int64).reshape(-1)
        self.rows = x.shape[0]
        self.base = D.Base(x, vocab, vec)
        self.X = x[:, :vocab].double().numpy()
        self.key = order_key(self.X)
        self.G = gumbel64(philox_words(self.seqs, vocab, self.seed, self.step))
        self._order = {}

    def order(self, r, allowed):
        """The allowed columns of row r by key descending, the lower column first among equals."""
        k = (r, allowed.tobytes())
        if k not in self._order:
            A = np.flatnonzero(allowed)
            self._order[k] = A[np.argsort(-self.key[r, A], kind="stable")]
        return self._order[k]

    def expected(self, M, T, top_k, top_p):
        """``M``: bool [rows, vocab], the mask every row takes."""
        M = np.asarray(M)
        e = Expected(self.rows)
        for r in range(self.rows):
            order = self.order(r, M[r])
            if order.size == 0:
                continue
            x, key = self.X[r], self.key[r]
            if not np.any(x[order] > -np.inf):
                e.token[r], e.n_kept[r] = int(order.min()), 1
                continue
            ks = key[order]
            nK = order.size
            if 0 < top_k < order.size:
                nK = int(np.count_nonzero(ks >= ks[top_k - 1]))
            n = nK
            score = x[order[:nK]] / T + self.G[r, order[:nK]]
            if top_p < 1.0:
                xk = x[order[:nK]]
                w = np.exp((xk - xk[0]) / T)
                w[np.isnan(w)] = 0.0
                cum = np.cumsum(w)
                Z = cum[-1]
                ends = np.flatnonzero(np.append(ks[1:nK] != ks[:nK - 1], True))
                Mend = cum[ends]
                j = int(np.argmax(Mend >= top_p * Z))
                n = int(ends[j]) + 1
                with np.errstate(invalid="ignore"):
                    rel = np.where(w > 0, 2 * U32 * (xk[0] - xk) / T + 2 * ACC_V_EXP * U32, 0.0)
                eps = 2 * (float((w * rel).sum()) / Z + nK * 2.0 ** -40) + 2.0 ** -39
                dist = np.abs(Mend / Z - top_p)
                e.worst_mass = min(e.worst_mass, float(dist.min() / eps))
                near = np.flatnonzero(dist <= eps)
                if near.size:
                    e.ambiguous[r] = True
                    for jj in set(near.tolist()) | {j}:
                        for q in (jj, min(jj + 1, ends.size - 1)):
                            m = int(ends[q]) + 1
                            e.alts[r][m] = _first_best(order[:m], score[:m])
            sc = np.where(np.isnan(score[:n]), -np.inf, score[:n])
            e.token[r], e.n_kept[r] = _first_best(order[:n], sc), n
            if n > 1:
                top2 = np.partition(sc, n - 2)[n - 2:]
                fin = np.isfinite(sc)
                g = np.abs(self.G[r, order[:n]][fin])
                delta = U32 * (np.abs(x[order[:n]][fin]) / T + np.abs(sc[fin])) + 2 * ACC_LOGF * U32 * (1 + np.maximum(g, 1.0))
                ratio = float(top2[1] - top2[0]) / (2 * float(delta.max())) if np.isfinite(top2[0]) else math.inf
                e.worst_margin = min(e.worst_margin, ratio)
                e.gap[r] = float(top2[1] - top2[0])
                e.margin_ok[r] = ratio > 1.0
        return e

    def logprob(self, token):
        """(float64 log-probability of ``token`` per row, its bound): 0 / 0 for token -1."""
        tok = torch.as_tensor(token, dtype=torch.int64)
        live = tok >= 0
        lp = self.base.X.gather(1, tok.clamp(min=0)[:, None])[:, 0] - self.base.lse
        zero = torch.zeros_like(lp)
        return torch.where(live, lp, zero), torch.where(live, self.base.dlse + U32 * lp.abs(), zero)


def judge(got, case, exp):
    """(token mismatches, n_kept mismatches, worst logprob err / bound, logprob misses) of the kernel's (token, logprob, n_kept).  An ambiguous
    row may report any of its neighbouring sets with that set's draw.  The log-probability is judged on the token the kernel reported."""
    tok, lp, kept = (t.detach().cpu() for t in got)
    bad_tok = bad_kept = 0
    for r in range(case.rows):
        t, n = int(tok[r]), int(kept[r])
        if exp.ambiguous[r] and n in exp.alts[r]:
            bad_tok += t != exp.alts[r][n]
        else:
            bad_tok += t != int(exp.token[r])
            bad_kept += n != int(exp.n_kept[r])
    ok = (tok >= 0) & (tok < case.vocab)
    elp, bound = case.logprob(torch.where(ok, tok, torch.full_like(tok, -1)))
    err = (lp.double() - elp).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    return int(bad_tok), int(bad_kept), float(ratio.max()), int((~(err <= bound)).sum())


# ---- the kernel in fp32, and its mutants ---------------------------------------------------------------------------------------------
def _f32(v):
    return np.float32(v)


def _fma32(a, b, c):
    return (a.astype(np.float64) * np.float64(b) + np.asarray(c, dtype=np.float64)).astype(np.float32)


def restate(x, vocab, M, *, T, top_k, top_p, seed, step, seqs, mutant=None):
    """decode_sample_kernel in fp32 numpy: the scores fma(x, fl(1 / T), G) with G through logf / log1pf of the 23-bit u, the masses
    exp2(fma(x, sc, nm)) 2^40 truncated to integers and summed as integers, the thresholds by count and by the integer compare
    M >= ceil(top_p Z), the draw with the lowest column on a tie.  Returns (token int64, logprob fp32, n_kept int64) as tensors.  ``mutant``
    plants one defect (MUTANTS)."""
    rows = x.shape[0]
    xf = x[:, :vocab].float().numpy()
    key = order_key(xf.astype(np.float64))
    seqs = torch.as_tensor(seqs, dtype=torch.int64).reshape(-1)
    words = philox_words(torch.zeros_like(seqs) if mutant == "sequence_ignored" else seqs, vocab, seed, step)
    if mutant == "u32":
        u = ((words.astype(np.float64) + 0.5) * 2.0 ** -32).astype(np.float32)           # rounds to 1.0 for the top 2^7 words
    else:
        u = (2 * (words >> 9) + 1).astype(np.float32) * _f32(2.0 ** -24)
    with np.errstate(divide="ignore", invalid="ignore"):
        l = np.where(u < _f32(0.5), -np.log(u), -np.log1p(u - _f32(1.0))).astype(np.float32)
        G = (-np.log(l)).astype(np.float32)
    inv_t, sc = _f32(1.0 / T), _f32(LOG2E / T)
    score = _fma32(xf, inv_t, G)
    tok, kept, lp = np.full(rows, -1, np.int64), np.full(rows, -1, np.int64), np.zeros(rows, np.float32)
    M = np.asarray(M)

    def cut_k(order, ks):
        if not 0 < top_k < order.size:
            return order
        return order[:top_k] if mutant == "ties_dropped" else order[:int(np.count_nonzero(ks >= ks[top_k - 1]))]

    def cut_p(r, order, ks):
        if not top_p < 1.0:
            return order
        with np.errstate(invalid="ignore", over="ignore"):
            nm = _f32(-xf[r, order[0]] * sc)
            w = np.exp2(_fma32(xf[r, order], sc, nm)).astype(np.float32)
            q = (np.where(w > 0, w, _f32(0)).astype(np.float64) * 2.0 ** 40).astype(np.int64)     # (w 2^40 is exact: a power of two)
        cum = np.cumsum(q)
        Z = int(cum[-1])
        target = min(max(int(math.ceil(top_p * float(Z))), 1), Z)
        ends = np.flatnonzero(np.append(ks[1:] != ks[:-1], True))
        hit = np.flatnonzero(cum[ends] >= target)
        return order[:int(ends[hit[0]]) + 1] if hit.size else order

    for r in range(rows):
        allowed = np.ones(vocab, dtype=bool) if mutant == "mask_ignored" else M[r]
        A = np.flatnonzero(allowed)
        if A.size == 0:
            continue
        xs = xf[r]
        if not np.any(xs[A] > -np.inf):
            tok[r], kept[r] = int(A.min()), 1
        else:
            order = A[np.argsort(-key[r, A], kind="stable")]
            if mutant == "topp_before_topk":
                order = cut_p(r, order, key[r, order])
                order = cut_k(order, key[r, order])
            else:
                order = cut_k(order, key[r, order])
                order = cut_p(r, order, key[r, order])
            tok[r], kept[r] = _first_best(order, score[r, order]), order.size
        xl = torch.from_numpy(xs / _f32(T)) if mutant == "temp_in_logprob" else torch.from_numpy(xs)
        if mutant == "mask_in_lse":
            xl = torch.where(torch.from_numpy(M[r]), xl, torch.full_like(xl, -math.inf))
        lp[r] = float(xl[tok[r]] - torch.logsumexp(xl, 0))
    return torch.from_numpy(tok), torch.from_numpy(lp), torch.from_numpy(kept)


# ---- the committed cases ---------------------------------------------------------------------------------------------------------------
SEEDS = {}      # (vocab, rows, dtype) -> attempt: filled by ``case``; the self-test asserts the conditions on what it finds
MAX_ATTEMPTS = 12


def masks_of(kind, vocab, rows):
    """(allow bool [vocab] or None, bool [rows, vocab])."""
    allow = D.make_mask(kind, vocab)
    return allow, D.row_masks(rows, vocab, allow, None, None, 0).numpy()


def conditions(case, exps):
    """Do the references of a case meet the issue's conditions?  Every row's draw margin; no ambiguous row at a vocabulary <= 2049, at most
    a quarter of a setting's rows at the flagship's."""
    for e in exps:
        if not e.margin_ok.all():
            return False
        limit = MAX_AMBIGUOUS_FLAGSHIP * case.rows if case.vocab == D.FLAGSHIP[0] else 0
        if e.ambiguous.sum() > limit:
            return False
    return True


@functools.lru_cache(maxsize=None)
def case(vocab, rows, dtype):
    """(Case, [(setting, allow, Expected)]) at the first of the seeds ``1000 a + vocab + rows`` (logits) / ``2^33 + a`` (Philox) whose
    references meet ``conditions``; the sequences are spread over the 32 bits, the step is 5."""
    ld = D.ld_of(vocab)
    for a in range(MAX_ATTEMPTS):
        x = D.make_logits(rows, vocab, ld, dtype, seed=1000 * a + vocab + rows)
        seqs = (torch.arange(rows, dtype=torch.int64) * 0x9E3779B1 + 3) & sr_ref.M32
        c = Case(x, vocab, seqs, seed=(1 << 33) + a, step=5)
        found = []
        for s in settings(vocab):
            allow, M = masks_of(s["kind"], vocab, rows)
            found.append((s, allow, c.expected(M, s["T"], s["top_k"], s["top_p"])))
        if conditions(c, [e for _, _, e in found]):
            SEEDS[(vocab, rows, dtype)] = a
            return c, found
    raise AssertionError(f"no seed in {MAX_ATTEMPTS} attempts meets the margin conditions at {vocab} x {rows} {dtype}")


SHAPES = [(v, 3) for v in VOCABS] + [(2049, 1), (2049, 257)]


def seq_words(seqs):
    """The int32 tensor the wrapper takes: the uint32 sequences, bit for bit."""
    s = torch.as_tensor(seqs, dtype=torch.int64) & sr_ref.M32
    return torch.where(s >= 2 ** 31, s - 2 ** 32, s).to(torch.int32)
