"""Parity of ``ssi_decode_select`` (csrc/decode_select.hip): a float64 reference of its three outputs, the bound of ``logprob`` derived from
the kernel's rounding points, an fp32 restatement of the kernel for the checker's CPU self-test, and the inputs, masks and planted rows that
tests/test_decode_select_ref.py (CPU) and tests/test_decode_select_gpu.py (GPU) share.  The role of tests/ce_parity.py, whose constants
(U32, the documented function accuracies) and helpers are used here.

Reference, on the STORED values (bf16 upcast to float64), per row with the mask the row takes (``early`` while ``n_generated < min_new``):
  token   = the lowest allowed column below vocab that holds the maximum over the allowed columns; -1 when nothing is allowed;
  logprob = x[token] - logsumexp(x[:vocab]) over ALL real columns; 0 for token -1;
  rank    = #{c < vocab: x[c] > x[token]} + #{c < token: x[c] == x[token]}; -1 for token -1.
``token`` and ``rank`` are exact integers.

The bound of ``logprob``, as ``Base.dlse`` of tests/ce_parity.py derives the register form's (the kernel forms its terms the same way):
term i of the exp-sum is exp2(fma(x_i, LOG2E, nm)), nm = fl(-gm LOG2E).  Against (x_i - gm) log2e the argument is off by U32 log2e |x_i - gm|
(LOG2E is an fp32 constant), U32 log2e |gm| (nm rounded) and U32 |argument| (the fma's one rounding): relatively, U32 (2 (gm - x_i) + |gm|)
plus v_exp_f32's 2 ACC_V_EXP U32 on the term; a term below 2^-126 may be flushed (vocab 2^-126 on a sum that is at least 1).  The sum's
longest chain of additions is ``chain`` long — a thread adds its own terms one by one, then two 6-level xor trees (the lanes of a wave, the
waves) — which adds chain U32 relatively (all terms are positive).  logf sees the sum's relative error r as the absolute -log1p(-r) and adds
its own 2 ACC_LOGF U32 |log sum|; gm + logf(sum) is one rounding, U32 |lse|; x[token] - lse the last one, U32 |logprob|.  x[token] and gm
are stored values: exact.  The output is fp32: that last rounding is the store."""
import math

import numpy as np
import torch

from ce_parity import ACC_LOGF, ACC_V_EXP, BF16, F32, TINY, U32, VEC, _L, _block_sum, _fma, cdiv

THREADS = 256
FLAGSHIP = (133_258, 133_376)                    # (vocab, ld) of the flagship model's head
VOCABS = (1, 7, 8, 9, 31, 32, 33, 255, 515, 2048, 2049, FLAGSHIP[0])
ROWS = (1, 3, 257)
MASK_KINDS = ("null", "ones", "bit0", "bit31", "bit32", "bitlast", "alternating", "block", "complement", "empty")
MUTANTS = ("mask_ignored", "mask_in_lse", "last_tie", "pad_counted", "early_at_equal", "word_bit_swap")
PADS = (float("nan"), float("inf"))              # the pad columns of row i: PADS[i % 2]
FAMILIES = ("randn", "ties", "shift60", "peaked")


def ld_of(vocab):
    """The smallest 16-byte aligned row with at least 3 pad columns (both dtypes take the vector path), or the flagship's."""
    return FLAGSHIP[1] if vocab == FLAGSHIP[0] else (vocab + 3 + 7) // 8 * 8


def vec_ok(ld, dtype):
    return (ld * (2 if dtype == BF16 else 4)) % 16 == 0


def make_logits(rows, vocab, ld, dtype, seed):
    """Row i is of family FAMILIES[i % 4]: 3 randn; integers in [-2, 2] (ties everywhere); 3 randn + 60 (a large |lse|); one column 30 above
    the rest.  Pad columns hold NaN (even rows) or +inf (odd rows)."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(rows, ld, generator=g)
    x = 3.0 * r
    for i in range(rows):
        fam = FAMILIES[i % 4]
        if fam == "ties":
            x[i] = torch.round(r[i].clamp(-2.4, 2.4))
        elif fam == "shift60":
            x[i] += 60.0
        elif fam == "peaked":
            x[i, int(r[i, :vocab].abs().argmax())] = x[i, :vocab].max() + 30.0
        x[i, vocab:] = PADS[i % 2]
    return x.to(dtype)


def make_mask(kind, vocab):
    """Bool [vocab], or None for the NULL mask; None also for a single bit that lies outside the vocabulary (the case does not exist)."""
    c = torch.arange(vocab)
    if kind == "null":
        return None
    if kind == "ones":
        return torch.ones(vocab, dtype=torch.bool)
    if kind.startswith("bit"):
        at = {"bit0": 0, "bit31": 31, "bit32": 32, "bitlast": vocab - 1}[kind]
        return c == at if at < vocab else None
    if kind == "alternating":
        return c % 2 == 1
    if kind in ("block", "complement"):
        blk = (c >= vocab // 4) & (c < vocab // 4 + max(1, vocab // 3))
        return blk if kind == "block" else ~blk
    if kind == "empty":
        return torch.zeros(vocab, dtype=torch.bool)
    raise ValueError(kind)


def mask_exists(kind, vocab):
    return kind in ("null",) or make_mask(kind, vocab) is not None


def pack(mask):
    """Bool [vocab] -> int32 words, bit c % 32 of word c // 32 (little-endian bit order, by numpy); None stays None."""
    if mask is None:
        return None
    words = cdiv(mask.numel(), 32)
    b = np.zeros(words * 32, dtype=np.uint8)
    b[:mask.numel()] = mask.numpy().astype(np.uint8)
    return torch.from_numpy(np.packbits(b, bitorder="little").view(np.uint32).astype(np.int64).astype(np.int32).copy())


def row_masks(rows, vocab, allow, early, n_gen, min_new):
    """Bool [rows, vocab]: the mask row r takes."""
    ones = torch.ones(vocab, dtype=torch.bool)
    a = ones if allow is None else allow
    e = ones if early is None else early
    use_early = torch.zeros(rows, dtype=torch.bool) if n_gen is None else n_gen.long() < min_new
    return torch.where(use_early[:, None], e[None, :], a[None, :])


def _first_max(X, M, last=False):
    """Per row the lowest (``last``: highest) column of M that holds the maximum of X over M; -1 for an empty M."""
    masked = torch.where(M, X, torch.full_like(X, -math.inf))
    mx = masked.max(1, keepdim=True).values
    hit = M & (masked == mx)
    col = torch.arange(X.shape[1])
    if last:
        tok = torch.where(hit, col[None, :], torch.full_like(col, -1)[None, :]).max(1).values
    else:
        tok = torch.where(hit, col[None, :], torch.full_like(col, X.shape[1])[None, :]).min(1).values
        tok = torch.where(tok == X.shape[1], torch.full_like(tok, -1), tok)
    return tok


def _rank(X, tok):
    xt = X.gather(1, tok.clamp(min=0)[:, None])
    col = torch.arange(X.shape[1])
    rk = (X > xt).sum(1) + ((X == xt) & (col[None, :] < tok[:, None])).sum(1)
    return torch.where(tok >= 0, rk, torch.full_like(rk, -1))


class Base:
    """What depends on the logits alone: shared by every mask of a case."""

    def __init__(self, x, vocab, vec=None):
        """``vec``: whether the kernel takes 16-byte loads on this input (None: from the row length; False for a base pointer off 16 bytes)."""
        self.x, self.vocab, self.dtype = x, vocab, x.dtype
        self.rows, self.ld = x.shape
        self.X = x[:, :vocab].double()
        self.gm = self.X.max(1).values
        self.lse = torch.logsumexp(self.X, 1)
        nvec = vocab // VEC[x.dtype] if (vec_ok(self.ld, x.dtype) if vec is None else vec) else 0
        self.chain = VEC[x.dtype] * cdiv(nvec, THREADS) + cdiv(vocab - nvec * VEC[x.dtype], THREADS) + 12
        p = torch.exp(self.X - self.lse[:, None])
        rel = U32 * (2 * (self.gm[:, None] - self.X) + self.gm.abs()[:, None]) + 2 * ACC_V_EXP * U32
        r = self.chain * U32 + (p * rel).sum(1) + vocab * TINY
        self.dlse = -torch.log1p(-r) + 2 * ACC_LOGF * U32 * (self.lse - self.gm).abs() + U32 * self.lse.abs()

    def expected(self, allow=None, early=None, n_gen=None, min_new=0):
        """(token int64, logprob float64, its bound, rank int64) per row."""
        M = row_masks(self.rows, self.vocab, allow, early, n_gen, min_new)
        tok = _first_max(self.X, M)
        live = tok >= 0
        lp = self.X.gather(1, tok.clamp(min=0)[:, None])[:, 0] - self.lse
        zero = torch.zeros_like(lp)
        return tok, torch.where(live, lp, zero), torch.where(live, self.dlse + U32 * lp.abs(), zero), _rank(self.X, tok)


def restate(x, vocab, allow_words=None, early_words=None, n_gen=None, min_new=0, mutant=None):
    """decode_select_kernel in fp32 torch from the PACKED masks: which mask a row takes, the bit of a column, the allowed first maximum (the
    kernel's merge order is immaterial where the values are totally ordered: no NaN), then the exp-sum with every thread adding ITS terms in
    the kernel's order — 16-byte vectors tid, tid + 256, ... and the scalar tail — and block_sum's two xor trees.  Returns (token, logprob
    fp32, rank).  ``mutant`` plants one defect (tests/test_decode_select_ref.py)."""
    rows, ld = x.shape
    dtype, N = x.dtype, VEC[x.dtype]
    width = vocab + 1 if (mutant == "pad_counted" and ld > vocab) else vocab       # the defect: column `vocab` counts everywhere
    col = torch.arange(width)

    def bits(words):
        if words is None:
            return torch.ones(width, dtype=torch.bool)
        w = words.long() & 0xffffffff
        if mutant == "word_bit_swap":
            wi, bi = col % 32, col // 32
        else:
            wi, bi = col // 32, col % 32
        ok = (wi < w.numel()) & (bi < 32)
        return ok & (((w[wi.clamp(max=w.numel() - 1)] >> bi.clamp(max=31)) & 1) == 1)

    if n_gen is None:
        use_early = torch.zeros(rows, dtype=torch.bool)
    else:
        use_early = n_gen.long() <= min_new if mutant == "early_at_equal" else n_gen.long() < min_new
    M = torch.where(use_early[:, None], bits(early_words)[None, :], bits(allow_words)[None, :])
    xf = x[:, :width].float()
    tok = _first_max(xf, torch.ones_like(M) if mutant == "mask_ignored" else M, last=mutant == "last_tie")
    live = tok >= 0
    xt = xf.gather(1, tok.clamp(min=0)[:, None])[:, 0]
    gm = xf.max(1).values
    nm = -gm * _L
    t = torch.exp2(_fma(xf, _L, nm[:, None]))
    if mutant == "mask_in_lse":
        t = torch.where(M, t, torch.zeros_like(t))
    nvec = width // N if vec_ok(ld, dtype) else 0
    J, tail = cdiv(nvec, THREADS), width - nvec * N
    s = torch.zeros(rows, THREADS, dtype=F32)
    if J:
        tv = torch.zeros(rows, J * THREADS * N, dtype=F32)
        tv[:, :nvec * N] = t[:, :nvec * N]
        tv = tv.view(rows, J, THREADS, N)
        for j in range(J):
            for e in range(N):
                s = s + tv[:, j, :, e]
    if tail:
        Jt = cdiv(tail, THREADS)
        tt = torch.zeros(rows, Jt * THREADS, dtype=F32)
        tt[:, :tail] = t[:, nvec * N:]
        tt = tt.view(rows, Jt, THREADS)
        for j in range(Jt):
            s = s + tt[:, j]
    lse = gm + torch.log(_block_sum(s))
    lp = torch.where(live, xt - lse, torch.zeros(rows, dtype=F32))
    return tok, lp, _rank(xf, tok)


def judge(got, exp):
    """(token mismatches, rank mismatches, worst logprob err / bound, logprob misses) of (token, logprob, rank) against ``Base.expected``."""
    tok, lp, rk = (t.detach().cpu() for t in got)
    etok, elp, bound, erk = exp
    err = (lp.double() - elp).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    return int((tok.long() != etok).sum()), int((rk.long() != erk).sum()), float(ratio.max()), int((~(err <= bound)).sum())


# ---- planted rows (vocab 2049: 16-byte vectors over [0, 2048), column 2048 is the scalar tail for both dtypes) -------------------------------
PLANT_VOCAB = 2049
# equal maxima at (a, b): neighbouring lanes of a wave for fp32 (thread = column // 4) and for bf16 (column // 8), two waves for either,
# two trips of one thread, and across the vector / tail boundary (thread 255 or 0's vector column against thread 0's tail column)
TIE_PAIRS = ((0, 4), (0, 8), (0, 256), (0, 512), (0, 1024), (3, 1027), (2047, 2048), (3, 2048))
PLANT_COUNT = 5


def tie_case(dtype, seed=11):
    """(x, list of (allow, expected token per row, expected rank per row)): row i holds the same value, above everything else, at TIE_PAIRS[i];
    with everything allowed the lower column wins (rank 0), with the lower one forbidden the higher (rank 1: one equal value before it), with
    the higher one forbidden the lower (rank 0)."""
    n = len(TIE_PAIRS)
    x = make_logits(n, PLANT_VOCAB, ld_of(PLANT_VOCAB), F32, seed).clamp(max=8.0)
    x[:, PLANT_VOCAB:] = torch.tensor([PADS[i % 2] for i in range(n)])[:, None]
    for i, (a, b) in enumerate(TIE_PAIRS):
        x[i, a] = x[i, b] = 9.0
    lo = torch.tensor([a for a, _ in TIE_PAIRS])
    hi = torch.tensor([b for _, b in TIE_PAIRS])
    settings = [(None, lo, torch.zeros(n, dtype=torch.int64))]
    for i, (a, b) in enumerate(TIE_PAIRS):           # one launch per forbidden column: the other rows see an ordinary mask
        for forbid, want, rank in ((a, b, 1), (b, a, 0)):
            allow = torch.ones(PLANT_VOCAB, dtype=torch.bool)
            allow[forbid] = False
            settings.append((allow, (i, want, rank)))
    return x.to(dtype), settings


def forbidden_max_case(dtype, seed=12):
    """(x, allow): in every row PLANT_COUNT forbidden columns (spread over lanes, waves and the tail) hold distinct values above every allowed
    one, so the chosen token's rank is exactly PLANT_COUNT."""
    rows = 4
    x = make_logits(rows, PLANT_VOCAB, ld_of(PLANT_VOCAB), F32, seed)
    cols = torch.tensor([1, 70, 700, 2040, 2048])
    assert len(cols) == PLANT_COUNT
    top = x[:, :PLANT_VOCAB].max(1).values
    for k, c in enumerate(cols.tolist()):
        x[:, c] = top + 8.0 * (k + 1)
    allow = torch.ones(PLANT_VOCAB, dtype=torch.bool)
    allow[cols] = False
    return x.to(dtype), allow


def min_new_case(dtype, seed=13):
    """(x, allow, early, n_gen, min_new): the row maximum is a "stop token" that ``early`` forbids; rows sit at min_new - 1 (early), min_new
    (not early), 0 (early) and far above."""
    vocab, min_new = 515, 4
    x = make_logits(4, vocab, ld_of(vocab), F32, seed)
    x[:, 77] = x[:, :vocab].max(1).values + 2.0
    allow = torch.ones(vocab, dtype=torch.bool)
    allow[100:200] = False
    early = allow.clone()
    early[77] = False
    return x.to(dtype), allow, early, torch.tensor([min_new - 1, min_new, 0, 1000], dtype=torch.int32), min_new
