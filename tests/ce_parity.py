"""Per-element parity of the cross-entropy kernels (csrc/embed_ce.hip, the five ``ssi_ce_fwd*`` entries in both forms): float64 references,
bounds derived from the rounding points of the two bodies, fp32 restatements of the bodies for the checker's CPU self-test, seeded inputs and the
shape / label tables.  Imported by tests/test_ce_parity_ref.py (CPU) and tests/test_ce_parity_gpu.py (GPU); the role of tests/attn_stress.py.

References follow include/ssi_hip.h on the STORED values (bf16 upcast to float64); a row whose label is ignored or outside [0, vocab) is 0 in
every output, rank -1.  ``teacher_lse`` is an input of ``ssi_ce_fwd_kl``: the references use the fp32 values the call is given, as the header's
formulas do (q = exp(t - teacher_lse)).

Bounds.  U32 = 2^-24 is one correctly rounded fp32 operation, a sum whose longest chain of additions is n long is off by at most
n U32 sum|terms| (Higham, Accuracy and Stability of Numerical Algorithms, 4.2: any order), ``ulp`` is the storage type's spacing with its
exponent held at -126.  The derivations stand beside the code (``dlse``, ``_grad_row_form``, ``_grad_generic``, ``expected``).  The four
function accuracies are DOCUMENTED values, not measured ones and not tuned (but for logf, raised after a traced measurement):

  ACC_V_EXP = 1 ulp  v_exp_f32   (``__builtin_amdgcn_exp2f``; CDNA ISA manual, transcendental instructions: 1 ulp)
  ACC_V_LOG = 1 ulp  v_log_f32   (``__log2f``; same table)
  ACC_EXPF  = 1 ulp  OCML expf   (ROCm OCML documentation, "Supported functions": expf 1 ulp)
  ACC_LOGF  = 3 ulp  OCML logf   (same: logf 1 ulp — measured 2.21 ulp in this build, see the constant)

Measured worst err / bound per family on an MI355X (form x mode; tests/test_ce_parity_gpu.py prints them at module end) are recorded in
profiles/LAB_NOTES.md and in the table at the end of this docstring.

  form         mode         grad row_loss  row_lse    row_z    row_u   row_kl  row_nll
  register     kl         0.9998   0.4944   0.4878        -        -   0.4014        -
  register     metrics         -   0.4944   0.4878        -        -        -   0.4621
  register     plain      0.9987   0.4944   0.4878        -        -        -        -
  register     smooth     1.0000   0.4944   0.4878   0.4248   0.2026        -        -
  register     z          0.9990   0.4944   0.4878   0.4248        -        -        -
  generic bf16 kl         0.9997   0.2508   0.2541        -        -   0.7730        -
  generic bf16 metrics         -   0.2508   0.2541        -        -        -   0.2454
  generic bf16 plain      0.9963   0.2508   0.2541        -        -        -        -
  generic bf16 smooth     0.9999   0.2508   0.2541   0.2517   0.1061        -        -
  generic bf16 z          0.9971   0.2508   0.2541   0.2517        -        -        -
  generic fp32 kl         0.7248   0.3229   0.3552        -        -   0.7546        -
  generic fp32 metrics         -   0.3229   0.3552        -        -        -   0.3375
  generic fp32 plain      0.3987   0.3229   0.3552        -        -        -        -
  generic fp32 smooth     0.4085   0.3229   0.3552   0.3063   0.1077        -        -
  generic fp32 z          0.3574   0.3229   0.3552   0.3063        -        -        -
"""
import math

import torch

BF16, F32 = torch.bfloat16, torch.float32
MANT = {BF16: 7, F32: 23}
VEC = {BF16: 8, F32: 4}
U32 = 2.0 ** -24
U64 = 2.0 ** -53
TINY = 2.0 ** -126
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2
LOG2E32 = float(torch.tensor(1.44269504088896340736, dtype=F32))   # the kernels' constant, as fp32 holds it
CHUNK = 8192
IGNORE = -100
SENTINEL = -7.25                                 # exact in bf16 (the guard rows)
# documented accuracies in ulp of fp32 (see the module docstring); 1 ulp is at most 2 U32 relative
ACC_V_EXP = 1.0
ACC_V_LOG = 1.0
ACC_EXPF = 1.0
# logf: RAISED AFTER MEASUREMENT from the documented 1.  Traced with a stand-alone sweep of logf over 65 536 arguments in [1, 1e6] against
# float64 on an MI355X, built with the library's flags: worst 2.21 ulp (2.92 U32 |logf|); 1.88 ulp with -ffp-contract=off.  The in-line
# expansion is v_log_f32 times ln 2 in extended precision: the instruction's 1 ulp of log2 y is up to 2 U32 relative, and stays that in
# ln y whatever its binade, before the product's own rounding and the fused product described below (logf's share of which is in the 2.21).
ACC_LOGF = 3.0
# What the build does to expf and logf (READ FROM THE COMPILED CODE, not measured and not tuned).  hipcc expands both in line with an
# extended-precision product: ph = fl(x c), pl = fma(x, c, -ph) + x c_tail (c = log2 e for expf, ln 2 after v_log_f32 for logf), then
# expf: exp2((ph - rint(ph)) + pl), logf: ph + pl.  Under the library's -ffp-contract=fast the backend fuses `ph - rint(ph)` and `ph + pl` with
# the product ph = x c into ONE fma on the exact product — which already holds the low part fma(x, c, -ph) that pl adds a second time.  The
# result is off by that low part, at most half an ulp of ph <= U32 |x c|: a relative U32 |x| more on expf(x) (ln 2 times it); logf's share is
# inside the measured ACC_LOGF.  Found by this suite: the fp32 generic CE_KL gradient at (vocab 515, ld 520), row 2, column 346, where the
# gradient is -bk q with q = expf(-16.466796875): 25.9 U32 from float64 against the 21.5 U32 that the subtraction's rounding (16.0 U32
# there), 1 ulp of expf and three fp32 operations allow; fp64 on the same argument puts 9.9 (+- 3) U32 on expf itself, and ln 2 times half an
# ulp of ph = -23.76 is up to 11.0 U32.  A stand-alone sweep of expf over [-87, 0] on an MI355X: worst 45.2 U32 (44 ulp) with the library's
# flags, (error - 2 U32) / (U32 |x|) at most 0.947; 0.81 ulp with -ffp-contract=off.  The raw v_exp_f32 / v_log_f32 of the register form
# are not affected (its lse takes logf, as the generic form's).
FUSED_EXPF = 1.0                                 # x U32 |x| relative on expf(x)
MAX_ELEMS = 24 * 147_456                         # all rows of a case


def cdiv(a, b):
    return -(-a // b)


def f32(v):
    return float(torch.tensor(v, dtype=F32))


# ---- which form an input takes: ce_row_form of csrc/embed_ce.hip, restated ----------------------------------------------------------------
def row_form(dtype, ld, vocab, aligned=True):
    chunks = cdiv(ld, CHUNK)
    return bool(dtype == BF16 and aligned and ld - vocab < CHUNK and ld * 2 < 2 ** 31 and (chunks <= 4 or chunks == 8 or 16 <= chunks <= 18))


# (vocab, ld, dtype, form, chunks): each the smallest ld of its class
_ROW = [(1, 515, 520), (1, 8192, 8192), (2, 8000, 8200), (2, 8193, 8200), (2, 16_384, 16_384), (3, 16_000, 16_392), (3, 20_000, 20_480),
        (4, 24_577, 24_584), (4, 32_768, 32_768), (4, 24_600, 32_760), (8, 57_345, 57_352), (8, 65_000, 65_536), (16, 122_881, 122_888),
        (17, 133_258, 133_376), (18, 139_265, 139_272), (18, 147_000, 147_456),
        (2, 515, 8704)]                          # pad 8189: the last pad width the register form takes
SHAPES = [(v, ld, BF16, "row", n) for n, v, ld in _ROW]
SHAPES += [(512, 8704, BF16, "generic", 2)]      # pad 8192: the generic form
SHAPES += [(515, 520, F32, "generic", 1), (9000, 9216, F32, "generic", 2)]
SHAPES += [(ld - 120, ld, BF16, "generic", n) for n, ld in ((5, 40_960), (7, 57_344), (9, 65_544), (15, 122_880), (19, 147_464))]
for _v, _ld, _dt, _form, _n in SHAPES:
    assert cdiv(_ld, CHUNK) == _n and _ld % 8 == 0 and _ld >= _v, (_v, _ld)
    assert row_form(_dt, _ld, _v) == (_form == "row"), (_v, _ld, _form)
ROW_NCH = sorted({s[4] for s in SHAPES if s[3] == "row"})
assert ROW_NCH == [1, 2, 3, 4, 8, 16, 17, 18]    # every instantiation of SSI_CE_DISPATCH_CHUNKS


def shape_id(s):
    return f"{s[0]}x{s[1]}-{'bf16' if s[2] == BF16 else 'fp32'}-{s[3]}{s[4]}"


def one_per_nch():
    """One register-form shape per chunk count (the one with pad columns where there is one) and every generic shape."""
    seen, out = set(), []
    for s in SHAPES:
        if s[3] == "row":
            if s[4] in seen or s[1] == s[0]:
                continue
            seen.add(s[4])
        out.append(s)
    return out


def case_rows(ld):
    return min(24, MAX_ELEMS // ld)


def is_valid(labels, vocab):
    return (labels != IGNORE) & (labels >= 0) & (labels < vocab)


def label_edges(vocab, ld):
    """0, vocab - 1 and, for every chunk c of the shape, c 8192 - 1, c 8192, c 8192 + 7, c 8192 + 8: the chunk, lane and within-register edges
    of the kernels' `hot` and `below`."""
    out = [0, vocab - 1]
    for c in range(cdiv(ld, CHUNK)):
        for lab in (c * CHUNK - 1, c * CHUNK, c * CHUNK + 7, c * CHUNK + 8):
            if 0 <= lab < vocab and lab not in out:
                out.append(lab)
    return out


def label_blocks(vocab, ld, rows=None, seed=0):
    """The label table cut into blocks of ``rows`` labels (a case's row budget).  EVERY block holds label 0, vocab - 1, one ignored label, one
    out of range above (vocab: a pad column's index) and one below; the chunk edges are dealt over the blocks; what is left of a block is
    filled with seeded labels."""
    rows = case_rows(ld) if rows is None else rows
    special = [0, vocab - 1, IGNORE, vocab, -7]
    edges = [e for e in label_edges(vocab, ld) if e not in special]
    per = rows - len(special)
    g = torch.Generator().manual_seed(seed + vocab)
    blocks = []
    for i in range(0, max(len(edges), 1), per):
        part = edges[i:i + per]
        fill = torch.randint(0, vocab, (per - len(part),), generator=g).tolist()
        body = part + fill
        # the specials at fixed rows inside the block: 0, 1 (row ends), 3 (ignored), 5 and rows - 1 (out of range)
        blk = [special[0], special[1], body[0], special[2], body[1], special[3]] + body[2:] + [special[4]]
        assert len(blk) == rows
        blocks.append(torch.tensor(blk, dtype=torch.int64))
    return blocks


def make_weights(rows, seed=0):
    """Weights in [0, 3] with an exact 0 (row 4, a labelled row) and an exact 1 (row 6)."""
    g = torch.Generator().manual_seed(seed + 17)
    w = 3.0 * torch.rand(rows, generator=g)
    if rows > 6:
        w[4], w[6] = 0.0, 1.0
    else:
        w[rows - 2], w[rows - 1] = 0.0, 1.0
    return w


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------------
FAMILIES = ("randn", "shift60", "shift40", "peaked")
MIXED = ("randn", "shift60", "shift40", "peaked", "randn")   # the family of row i of a mixed buffer: MIXED[i % 5]
PADS = (float("nan"), 1e4, float("inf"))                     # the student's pad columns of row i: PADS[i % 3]
TEACHER_PADS = (-3e4, float("nan"))                          # the teacher's: TEACHER_PADS[i % 2]


def _family_row(fam, r, vocab):
    if fam == "randn":
        return 3.0 * r
    if fam == "shift60":                         # a large |lse|: the rounding of nl = -lse log2e + log2 w matters
        return 3.0 * r + 60.0
    if fam == "shift40":                         # lse < -1 / (2 z) at z = 0.5: f < 0
        return 10.0 * r - 40.0
    if fam == "peaked":                          # one column 30 above the rest: probabilities over 13 decades
        x = 3.0 * r
        j = int(r[:vocab].abs().argmax())        # a seeded column
        x[j] = x[:vocab].max() + 30.0
        return x
    if fam == "ties":                            # integer logits in [-2, 2]: the rank's tie rule
        return torch.round(r.clamp(-2.4, 2.4))
    raise ValueError(fam)


def make_logits(rows, vocab, ld, dtype, seed, families=MIXED, pads=PADS):
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(rows, ld, generator=g)
    x = torch.empty(rows, ld)
    for i in range(rows):
        x[i] = _family_row(families[i % len(families)], r[i], vocab)
        x[i, vocab:] = pads[i % len(pads)]
    return x.to(dtype)


def make_teacher(logits, vocab, kind, seed, pads=TEACHER_PADS):
    """``near``: the student + 0.5 randn; ``far``: an independent 3 randn (tests/test_ce_kl_gpu.py's two)."""
    g = torch.Generator().manual_seed(seed + 1002)
    n = torch.randn(logits.shape, generator=g)
    t = logits.float() + 0.5 * n if kind == "near" else 3.0 * n
    for i in range(t.shape[0]):
        t[i, vocab:] = pads[i % len(pads)]
    return t.to(logits.dtype)


# ---- the modes a case runs -------------------------------------------------------------------------------------------------------------------
def mode(kind, z=0.0, e=0.0, beta=0.0, teacher=None, kw=False):
    return dict(kind=kind, z=z, e=e, beta=beta, teacher=teacher, kw=kw)


MODES = [mode("plain"), mode("z", z=1e-4), mode("z", z=0.5), mode("smooth", e=0.1), mode("smooth", e=0.1, z=1e-4), mode("metrics"),
         mode("kl", beta=0.1, teacher="near"), mode("kl", beta=2.0, teacher="far", kw=True), mode("kl", beta=0.1, teacher="far", kw=True),
         mode("kl", beta=2.0, teacher="near")]


def mode_id(m):
    s = m["kind"]
    if m["kind"] in ("z", "smooth") and (m["z"] or m["kind"] == "z"):
        s += f"-z{m['z']:g}"
    if m["kind"] == "smooth":
        s += f"-e{m['e']:g}"
    if m["kind"] == "kl":
        s += f"-b{m['beta']:g}-{m['teacher']}" + ("-kw" if m["kw"] else "")
    return s


# ---- float64 references and bounds -----------------------------------------------------------------------------------------------------------
def ulp(ref, dtype):
    """Spacing of `dtype` at |ref| (float64): 2^(floor(log2 |ref|) - mantissa bits), the exponent held at -126."""
    _, ex = torch.frexp(ref.abs())
    ex = torch.where(ref == 0, torch.full_like(ex, -1000), ex)
    return torch.ldexp(torch.ones_like(ref), (ex - 1).clamp(min=-126) - MANT[dtype])


def stored(ref, err, dtype):
    """`err` arrives at the one store; the store adds half an ulp of the storage type at |ref| + err.  Below the smallest normal a flushed 0
    is accepted: the bound is at least |ref| there."""
    b = err + 0.5 * ulp(ref.abs() + err, dtype)
    return torch.where(ref.abs() < 2 * TINY, torch.maximum(b, ref.abs()), b)


class Base:
    """What depends on the logits alone: shared by every mode and label block of a case."""

    def __init__(self, x, vocab):
        self.x, self.vocab, self.dtype = x, vocab, x.dtype
        self.rows, self.ld = x.shape
        self.X = x[:, :vocab].double()
        self.gm = self.X.max(1).values
        self.lse = torch.logsumexp(self.X, 1)
        self.p = torch.exp(self.X - self.lse[:, None])
        self.nch = cdiv(self.ld, CHUNK)
        self.vpt = cdiv(self.ld // VEC[x.dtype], 512)     # generic form: 16-byte vectors per thread
        self._dlse = {}

    def chain(self, form):
        """Longest chain of additions of a row sum.  Register form: a lane adds its 8 NCH terms, then two 6-level xor trees (the lanes of a
        wave, the 16 waves).  Generic form: a thread adds its N vpt terms, then the same two trees."""
        return (8 * self.nch if form == "row" else VEC[self.dtype] * self.vpt) + 12

    def dlse(self, form):
        """|lse_kernel - lse| per row.
        Register form: term i of the exp-sum is exp2(fma(x_i, LOG2E, nm)), nm = fl(-gm LOG2E).  Against (x_i - gm) log2e the argument is off
        by U32 log2e |x_i - gm| (LOG2E is an fp32 constant), U32 log2e |gm| (nm rounded) and U32 |argument| (the fma's one rounding); the
        term's relative error is ln 2 times that plus v_exp_f32's.  The sum adds chain U32; logf sees the sum's relative error as an
        absolute one and adds its own; gm + logf(gs) is one more rounding.
        Generic form: a thread's running max m rises through m_1 < m_2 < ...; each rise multiplies the sum by expf(fl(m_k - m_k+1)) — the
        argument roundings add up to U32 (m_last - m_first) <= U32 R, R the row's range, and each of at most vpt + 1 factors (the last one to
        the block's max) costs expf's error and one multiply; a term is expf(fl(x - m)): U32 R and expf's error again.  The fused product
        inside expf (FUSED_EXPF) costs U32 |argument| wherever an argument's rounding does: 2 U32 R more."""
        if form not in self._dlse:
            n = self.chain(form) * U32
            if form == "row":
                rel = U32 * (2 * (self.gm[:, None] - self.X) + self.gm.abs()[:, None]) + 2 * ACC_V_EXP * U32
                r = n + (self.p * rel).sum(1) + self.vocab * TINY          # (p_i = term_i / sum; a flushed term is off by < 2^-126)
            else:
                R = self.gm - self.X.min(1).values
                r = n + 2 * (1 + FUSED_EXPF) * U32 * R + (self.vpt + 2) * (2 * ACC_EXPF + 1) * U32
            loggs = self.lse - self.gm
            self._dlse[form] = -torch.log1p(-r) + 2 * ACC_LOGF * U32 * loggs.abs() + U32 * self.lse.abs()
        return self._dlse[form]


def _rel_f(f, two_z, dl):
    """f = fma(two_z, lse, 1) with the kernel's lse: off by two_z dl + U32 |f|; as a relative error of |f| (inf where that reaches 1/2)."""
    r = (two_z * dl + U32 * f.abs()) / f.abs()
    assert bool((r < 0.5).all()), "an input row with f = 1 + 2 z lse at 0: its bound would be empty"
    return torch.where(r < 0.5, -torch.log1p(-r.clamp(max=0.5)), torch.full_like(r, float("inf")))


def _grad_row_form(b, kind, wd, wgiven, f, two_z, ome, wu, onehot, valid, bk=None, T=None, tlse=None):
    """The gradient row of ce_row_bf16_body and its bound.  P = s p is ONE exp2: exp2(fma(x, LOG2E, nl)), nl = fma(-lse, LOG2E, log2 s_w)
    [+ log2 |f|], s = w |f| (CE_KL: w + bk).  The argument's absolute error against (x - lse) log2e + log2 s:
      U32 log2e |x - lse|   LOG2E as fp32 (x LOG2E - lse LOG2E share it)
      log2e dlse            the kernel's lse
      2 ACC_V_LOG U32 |log2 s_w|   __log2f (none without weights: log2w is the constant 0)
      [CE_KL] 2 U32 log2e   bk = beta k and w + bk, one rounding each
      U32 |nl|              the fma that forms nl
      [f] log2e rel_f, 2 ACC_V_LOG U32 |log2 |f||, U32 |nl + log2 |f||     f itself, its __log2f, the add
      U32 |argument|        the element's fma
    P's relative error is expm1(ln 2 times that) plus v_exp_f32's; a P below 2^-126 may come out 0.  Then one U32 per further fp32
    operation on its result (the label's subtraction; - wus; - bk q with q's own error and bk's), wl = w ome and wus = w e/V two roundings
    each, then the ONE store to bf16.  The sign of f is applied to the packed result: round-to-nearest is symmetric, nothing to add."""
    X, lse, p, dl = b.X, b.lse, b.p, b.dlse("row")
    sw = wd if bk is None else wd + bk
    log2sw = torch.where(sw > 0, torch.log2(sw.clamp(min=TINY)), torch.zeros_like(sw))
    nl = -lse * LOG2E + log2sw
    d = LOG2E * dl + U32 * nl.abs()
    if wgiven or bk is not None:
        d = d + 2 * ACC_V_LOG * U32 * log2sw.abs()
    if bk is not None:
        d = d + 2 * U32 * LOG2E
    s = sw
    if kind in ("z", "smooth"):
        log2f = torch.log2(f.abs())
        d = d + LOG2E * _rel_f(f, two_z, dl) + 2 * ACC_V_LOG * U32 * log2f.abs() + U32 * (nl + log2f).abs()
        s = sw * f.abs()
    log2s = torch.where(s > 0, torch.log2(s.clamp(min=TINY)), torch.zeros_like(s))
    arg = (X - lse[:, None]) * LOG2E + log2s[:, None]
    d_el = d[:, None] + U32 * LOG2E * (X - lse[:, None]).abs() + U32 * arg.abs()
    P = s[:, None] * p
    EP = P * (torch.expm1(LN2 * d_el) + 2 * ACC_V_EXP * U32) + torch.where(P < 2 * TINY, P, torch.zeros_like(P))
    sgn = torch.sign(f) if kind in ("z", "smooth") else torch.ones_like(wd)
    G = sgn[:, None] * P - (wd * ome)[:, None] * onehot
    E = EP + onehot * (U32 * (P - (wd * ome)[:, None]).abs() + (2 * U32 * wd * ome)[:, None] * (1.0 if kind == "smooth" else 0.0))
    if kind == "smooth":
        G = G - wu[:, None]
        E = E + U32 * G.abs() + 2 * U32 * wu[:, None]
    if bk is not None:
        # q = exp2(fma(t, LOG2E, nq)), nq = fl(-tlse LOG2E): as a term of the exp-sum, with tlse for gm
        dq = U32 * LOG2E * (2 * (T - tlse[:, None]).abs() + tlse.abs()[:, None])
        q = torch.exp(T - tlse[:, None])
        rq = torch.expm1(LN2 * dq) + 2 * ACC_V_EXP * U32
        G = G - bk[:, None] * q
        E = E + bk[:, None] * (q * (rq + 2 * U32) + torch.where(q < 2 * TINY, q, torch.zeros_like(q))) + U32 * G.abs()
    vz = valid[:, None]
    return torch.where(vz, G, torch.zeros_like(G)), torch.where(vz, stored(G, E, BF16), torch.zeros_like(G))


def _grad_generic(b, kind, wd, f, two_z, ome, wu, onehot, valid, bk=None, T=None, tlse=None):
    """The gradient row of ce_generic_body.  p = expf(fl(x - lse)): the argument is off by U32 |x - lse| and dlse, p by expm1 of that plus
    expf's error (1 ulp, and FUSED_EXPF U32 |x - lse| for the fused product inside it).  CE_PLAIN  w (p - onehot): the subtraction and the
    product, one U32 each.  CE_Z / CE_SMOOTH  w (f p - ome onehot) [- wu]: f's own error, the product f p, the subtraction, the product with w, [ome = 1 - e, wu = w (e / V) two roundings, the last subtraction].
    CE_KL  w (p - onehot) + bk (p - q): q = expf(fl(t - tlse)) likewise (tlse is an input: exact), bk = beta k one rounding, two products,
    two subtractions, one sum.  (-ffp-contract=fast may fuse a product into the next add: one rounding fewer, never more.)  Then ONE store."""
    X, lse, p, dl = b.X, b.lse, b.p, b.dlse("generic")
    rp = torch.expm1((1 + FUSED_EXPF) * U32 * (X - lse[:, None]).abs() + dl[:, None]) + 2 * ACC_EXPF * U32
    w_ = wd[:, None]
    if kind == "plain":
        G = w_ * (p - onehot)
        E = w_ * (p * rp + U32 * (p - onehot).abs()) + U32 * G.abs()
    elif kind in ("z", "smooth"):
        f_, o_ = f[:, None], ome * onehot
        inner = f_ * p - o_
        G = w_ * inner
        E = w_ * (f_.abs() * p * (rp + _rel_f(f, two_z, dl)[:, None] + U32) + U32 * inner.abs() + U32 * o_) + U32 * G.abs()
        if kind == "smooth":
            G = G - wu[:, None]
            E = E + 2 * U32 * wu[:, None] + U32 * G.abs()
    else:
        bk_ = bk[:, None]
        q = torch.exp(T - tlse[:, None])
        rq = torch.expm1((1 + FUSED_EXPF) * U32 * (T - tlse[:, None]).abs()) + 2 * ACC_EXPF * U32
        a, c = w_ * (p - onehot), bk_ * (p - q)
        G = a + c
        E = w_ * (p * rp + U32 * (p - onehot).abs()) + U32 * a.abs() + bk_ * (p * rp + q * rq + U32 * (p - q).abs()) + 2 * U32 * c.abs() \
            + U32 * G.abs()
    vz = valid[:, None]
    return torch.where(vz, G, torch.zeros_like(G)), torch.where(vz, stored(G, E, b.dtype), torch.zeros_like(G))


def expected(base, labels, m, form, w=None, teacher=None, tlse=None, k=None):
    """{output: (float64 reference, bound)} of one call: mode ``m`` (an entry of MODES) in ``form`` ("row" / "generic") on ``base``'s logits.
    ``grad`` is [rows, vocab]; ``row_rank`` is an exact int64 with bound None.  ``tlse``: the fp32 teacher_lse the call is given."""
    b, kind, vocab = base, m["kind"], base.vocab
    X, lse = b.X, b.lse
    valid = is_valid(labels, vocab)
    lab = labels.clamp(0, vocab - 1)
    xl = X.gather(1, lab[:, None])[:, 0]
    wd = torch.ones(b.rows, dtype=torch.float64) if w is None else w.double()
    dl = b.dlse(form)
    zero = torch.zeros_like(lse)
    out = {}

    def put(name, ref, bound):
        out[name] = (torch.where(valid, ref, zero), torch.where(valid, bound, zero))

    nll = lse - xl
    put("row_lse", lse, dl)
    # row_loss = fl(w fl(lse - xl)): the kernel's lse, the subtraction, the product
    put("row_loss", wd * nll, wd * (dl + U32 * nll.abs()) + U32 * (wd * nll).abs())
    two_z = 2.0 * f32(m["z"])
    f = 1.0 + two_z * lse
    e32 = f32(m["e"])
    ome = 1.0 - e32
    wu = wd * (e32 / vocab)
    onehot = torch.zeros_like(X)
    onehot[valid, lab[valid]] = 1.0
    if kind in ("z", "smooth"):
        # row_z = fl(w fl(lse lse))
        put("row_z", wd * lse * lse, wd * (2 * lse.abs() * dl + dl * dl + U32 * lse * lse) + U32 * (wd * lse * lse).abs())
    if kind == "smooth":
        # row_u = fl(w fl(lse - fl(sx / V))): sx a plain sum over vocab terms (chain U32 sum |x|), the division, the subtraction, the product
        mean = X.mean(1)
        u = wd * (lse - mean)
        put("row_u", u, wd * (dl + b.chain(form) * U32 * X.abs().sum(1) / vocab + U32 * mean.abs() + U32 * (lse - mean).abs()) + U32 * u.abs())
    if kind == "metrics":
        put("row_nll", nll, dl + U32 * nll.abs())
        col = torch.arange(vocab)
        rank = (X > xl[:, None]).sum(1) + ((X == xl[:, None]) & (col[None, :] < labels[:, None])).sum(1)
        out["row_rank"] = (torch.where(valid, rank, torch.full_like(rank, -1)), None)
        return out
    bk = T = tl = None
    if kind == "kl":
        kd = wd if k is None else k.double()
        bk = f32(m["beta"]) * kd
        T, tl = teacher[:, :vocab].double(), tlse.double()
        q = torch.exp(T - tl[:, None])
        dlr = tl - lse
        inner = (T - X) - dlr[:, None]
        if form == "row":
            # the fp32 sum of q ((t - x) - (tlse - lse)) over vocab terms: q's error (as in the gradient), the roundings of t - x, of
            # tlse - lse (which carries dlse), of the subtraction and of the product, the chain, the product with k
            dq = U32 * LOG2E * (2 * (T - tl[:, None]).abs() + tl.abs()[:, None])
            rq = torch.expm1(LN2 * dq) + 2 * ACC_V_EXP * U32
            ref = kd * (q * inner).sum(1)
            err = (q * (rq * inner.abs() + U32 * ((T - X).abs() + dlr.abs()[:, None] + 2 * inner.abs()) + dl[:, None])).sum(1) \
                + b.chain(form) * U32 * (q * inner.abs()).sum(1)
            put("row_kl", ref, kd * err + U32 * ref.abs())
        else:
            # the fp64 form of the header: both fp32 lse drop out (log S, log SP); what is left is fp64 rounding over vocab terms, the
            # conversion to fp32 and the product with k
            qs = torch.softmax(T, 1)
            ref = kd * (qs * (torch.log_softmax(T, 1) - torch.log_softmax(X, 1))).sum(1)
            slack = (vocab / 512 + 16) * 2 * U64 * ((qs * (T - X).abs()).sum(1) + tl.abs() + lse.abs() + 2)
            put("row_kl", ref, 2 * U32 * ref.abs() + kd * slack)
    if form == "row":
        out["grad"] = _grad_row_form(b, kind, wd, w is not None, f, two_z, ome, wu, onehot, valid, bk, T, tl)
    else:
        out["grad"] = _grad_generic(b, kind, wd, f, two_z, ome, wu, onehot, valid, bk, T, tl)
    return out


def ratio(got, ref, bound):
    """(worst err / bound, its index, number of elements that miss) over EVERY element; NaN / inf in `got` miss."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    i = int(r.argmax())
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), r.shape)) if r.dim() > 1 else (i,)
    return float(r.flatten()[i]), idx, int((~(err <= bound)).sum())


def old_gradient_passes(got, ref, scale):
    """The gradient tolerance of the older files in bf16: atol 4e-3 max(1, scale) + rtol 1e-2 |ref|; the elements that pass."""
    return (got.double() - ref).abs() <= 4e-3 * scale.clamp(min=1.0)[:, None] + 1e-2 * ref.abs()


# ---- fp32 restatements of the two bodies (CPU self-test only) -------------------------------------------------------------------------------
_L = torch.tensor(LOG2E32, dtype=F32)


def _fma(a, b, c):
    """fp32 fma through float64 (the product of two fp32 is exact there)."""
    return (a.double() * b.double() + c.double()).float()


def _xor_tree(v):
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ o]
    return v[..., 0]


def _block_sum(s):
    """block_sum of common_hip.h: the xor tree over a wave's 64 lanes, then the same tree over the waves' results (0 beyond them)."""
    rows, t = s.shape
    wv = _xor_tree(s.view(rows, t // 64, 64))
    pad = torch.zeros(rows, 64, dtype=s.dtype)
    pad[:, :t // 64] = wv
    return _xor_tree(pad)


def _scalars(m, vocab):
    z32, e32 = torch.tensor(m["z"], dtype=F32), torch.tensor(m["e"], dtype=F32)
    return 2.0 * z32, 1.0 - e32, e32 / torch.tensor(float(vocab), dtype=F32), torch.tensor(m["beta"], dtype=F32)


def restate_row_form(x, labels, vocab, m, w=None, teacher=None, tlse=None, k=None, mutant=None):
    """ce_row_bf16_body in fp32 torch: the masking, max, exp-sum (per lane over its 4 NCH packed pairs, then block_sum), lse, the scalars and
    the gradient loop, statement by statement.  Returns {row_loss, row_lse, row_z, row_u, row_nll, row_rank, row_kl, grad [rows, ld] in bf16}.
    ``mutant`` plants one defect (tests/test_ce_parity_ref.py)."""
    kind = m["kind"]
    rows, ld = x.shape
    nch = cdiv(ld, CHUNK)
    W = nch * CHUNK
    two_z, ome, e_over_v, beta = _scalars(m, vocab)
    col = torch.arange(W)
    real = col < vocab

    def load(buf):
        r = torch.zeros(rows, W, dtype=F32)      # loads beyond the row return 0
        r[:, :ld] = buf.float()
        return r

    xr = load(x)
    if mutant == "swap_chunks":
        xr[0, :2 * CHUNK] = torch.cat([xr[0, CHUNK:2 * CHUNK], xr[0, :CHUNK]])
    raw = xr.clone()
    xr[:, ~real] = -math.inf
    xs = xr
    if mutant == "pad_in_sum":
        xs = xr.clone()
        xs[:, vocab] = 0.0
    valid = is_valid(labels, vocab)
    lab = labels.clamp(0, vocab - 1)
    wv = torch.ones(rows, dtype=F32) if (w is None or mutant == "drop_weight") else w.float()
    xl = x.float().gather(1, lab[:, None])[:, 0]
    gm = xs.max(1).values
    nm = -gm * _L
    t = torch.exp2(_fma(xs, _L, nm[:, None])).view(rows, nch, 1024, 4, 2)
    pair = t[..., 0] + t[..., 1]
    s = torch.zeros(rows, 1024, dtype=F32)
    for c in range(nch):
        for d in range(4):
            s = s + pair[:, c, :, d]
    lse = gm + torch.log(_block_sum(s))
    out = {}
    vz = valid.float()
    out["row_loss"], out["row_lse"] = wv * (lse - xl) * vz, lse * vz
    out["row_z"] = wv * (lse * lse) * vz
    if kind == "smooth":
        v = torch.where(real, xr, torch.zeros_like(xr))
        if mutant == "u_over_ld":
            v = torch.where(col < ld, raw, torch.zeros_like(raw))
        v = v.view(rows, nch, 1024, 4, 2)
        vp = v[..., 0] + v[..., 1]
        sx = torch.zeros(rows, 1024, dtype=F32)
        for c in range(nch):
            for d in range(4):
                sx = sx + vp[:, c, :, d]
        out["row_u"] = wv * (lse - _block_sum(sx) / float(vocab)) * vz
    if kind == "metrics":
        below = col[None, :] <= labels[:, None] if mutant == "rank_le" else col[None, :] < labels[:, None]
        cnt = ((xr > xl[:, None]) | ((xr == xl[:, None]) & below)).sum(1)
        out["row_nll"] = (lse - xl) * vz
        out["row_rank"] = torch.where(valid, cnt, torch.full_like(cnt, -1))
        return out
    log2w = torch.log2(wv) if w is not None else torch.zeros(rows, dtype=F32)
    bk = torch.zeros(rows, dtype=F32)
    if kind == "kl":
        kw = wv if k is None else k.float()
        bk = torch.where(valid, beta * kw, torch.zeros_like(kw))
        log2w = torch.log2(wv + bk)
        tl = tlse.float()
        dl = tl - lse
        nq = torch.where(valid, -tl * _L, torch.full_like(tl, -math.inf))
    nl = _fma(-lse, _L, log2w)
    wl, wus = wv.clone(), torch.zeros(rows, dtype=F32)
    neg = torch.zeros(rows, dtype=torch.bool)
    if kind in ("z", "smooth"):
        f = _fma(two_z, lse, torch.ones(rows, dtype=F32))
        nl = nl + torch.log2(f.abs())
        if kind == "smooth":
            wl, wus = wv * ome, wv * e_over_v
        neg = (f < 0) & valid
        wl, wus = torch.where(neg, -wl, wl), torch.where(neg, -wus, wus)
    nl = torch.where(valid, nl, torch.full_like(nl, -math.inf))
    wus = torch.where(valid, wus, torch.zeros_like(wus))
    g = torch.exp2(_fma(xr, _L, nl[:, None]))
    if mutant == "double_round":
        g = g.to(BF16).float()
    hot = torch.zeros(rows, W, dtype=torch.bool)
    hot[valid, lab[valid]] = True
    g = g - torch.where(hot, wl[:, None].expand(rows, W), torch.zeros(rows, W))
    if kind == "smooth" and mutant != "drop_wu":
        g = g - torch.where(real[None, :], wus[:, None].expand(rows, W), torch.zeros(rows, W))
    if kind == "kl":
        te = load(teacher)
        if mutant == "teacher_early":            # the ring register never refilled: chunk c >= TD reads what chunk c - TD left there
            td = min(nch, 3)
            tv = te.view(rows, nch, CHUNK)
            te = torch.stack([tv[:, c if c < td else c - td] for c in range(nch)], 1).reshape(rows, W)
        te = torch.where(valid[:, None], te, torch.zeros_like(te))
        q = torch.exp2(_fma(te, _L, nq[:, None]))
        term = q * ((te - xr) - dl[:, None])
        q = torch.where(real[None, :], q, torch.zeros_like(q))
        term = torch.where(real[None, :], term, torch.zeros_like(term)).view(rows, nch, 1024, 8)
        acc = torch.zeros(rows, 1024, dtype=F32)
        for c in range(nch):
            for e in range(8):
                acc = acc + term[:, c, :, e]
        out["row_kl"] = torch.where(valid, kw * _block_sum(acc), torch.zeros(rows, dtype=F32))
        g = g - bk[:, None] * q
    if mutant == "zero_nonlabel":
        g = torch.where(hot, g, torch.zeros_like(g))
    gb = g.to(BF16)
    gb = torch.where(neg[:, None], -gb, gb)      # the sign bit of the packed result (zeros become -0)
    out["grad"] = gb[:, :ld]
    return out


def restate_generic(x, labels, vocab, m, w=None, teacher=None, tlse=None, k=None):
    """ce_generic_body in fp32 torch: 512 threads stride over the row's 16-byte vectors with an online max / sum, block_max / block_sum, the
    gradient from a second pass; CE_KL sums in fp64.  Same outputs as ``restate_row_form``, the gradient in the storage type."""
    kind, dtype = m["kind"], x.dtype
    rows, ld = x.shape
    N = VEC[dtype]
    K = cdiv(ld // N, 512)
    W = K * 512 * N
    two_z, ome, e_over_v, beta = _scalars(m, vocab)
    col = torch.arange(W)
    real = col < vocab
    xr = torch.zeros(rows, W, dtype=F32)
    xr[:, :ld] = x.float()
    xv, ok = xr.view(rows, K, 512, N), real.view(K, 512, N)
    ninf = torch.tensor(-math.inf, dtype=F32)
    mx = torch.full((rows, 512), -math.inf, dtype=F32)
    s = torch.zeros(rows, 512, dtype=F32)
    sx = torch.zeros(rows, 512, dtype=F32)
    for kk in range(K):
        a, o = xv[:, kk], ok[kk]
        lm = torch.where(o[None], a, ninf).max(-1).values
        upd = lm > mx
        s = torch.where(upd, s * torch.exp(mx - lm), s)
        mx = torch.where(upd, lm, mx)
        for i in range(N):
            s = s + torch.where(o[None, :, i], torch.exp(a[..., i] - mx), torch.zeros_like(s))
            sx = sx + torch.where(o[None, :, i], a[..., i], torch.zeros_like(s))
    gm = mx.max(1).values
    s = torch.where(mx == -math.inf, torch.zeros_like(s), s * torch.exp(mx - gm[:, None]))
    lse = gm + torch.log(_block_sum(s))
    valid = is_valid(labels, vocab)
    lab = labels.clamp(0, vocab - 1)
    wv = torch.ones(rows, dtype=F32) if w is None else w.float()
    xl = x.float().gather(1, lab[:, None])[:, 0]
    vz = valid.float()
    out = {"row_loss": wv * (lse - xl) * vz, "row_lse": lse * vz, "row_z": wv * (lse * lse) * vz}
    if kind == "smooth":
        out["row_u"] = wv * (lse - _block_sum(sx) / float(vocab)) * vz
    X = xr[:, :vocab]
    if kind == "metrics":
        c = torch.arange(vocab)
        cnt = ((X > xl[:, None]) | ((X == xl[:, None]) & (c[None, :] < labels[:, None]))).sum(1)
        out["row_nll"] = (lse - xl) * vz
        out["row_rank"] = torch.where(valid, cnt, torch.full_like(cnt, -1))
        return out
    onehot = torch.zeros(rows, vocab, dtype=F32)
    onehot[valid, lab[valid]] = 1.0
    p = torch.exp(X - lse[:, None])
    if kind == "plain":
        g = wv[:, None] * (p - onehot)
    elif kind in ("z", "smooth"):
        f = _fma(two_z, lse, torch.ones(rows, dtype=F32))
        g = wv[:, None] * (f[:, None] * p - ome * onehot)
        if kind == "smooth":
            g = g - (wv * e_over_v)[:, None]
    else:
        kw = wv if k is None else k.float()
        bk = beta * kw
        tl = tlse.float()
        Tt = teacher.float()[:, :vocab]
        q = torch.exp(Tt - tl[:, None])
        g = wv[:, None] * (p - onehot) + bk[:, None] * (p - q)
        T64, X64, tl64, l64 = Tt.double(), X.double(), tl.double(), lse.double()
        Q = torch.exp(T64 - tl64[:, None])
        s0, s1, s2 = (Q * (T64 - X64)).sum(1), Q.sum(1), torch.exp(X64 - l64[:, None]).sum(1)
        out["row_kl"] = kw * (s0 / s1 - (tl64 - l64) - torch.log(s1) + torch.log(s2)).float() * vz
    full = torch.zeros(rows, ld, dtype=F32)
    full[:, :vocab] = g * vz[:, None]
    out["grad"] = full.to(dtype)
    return out


def restate(form, *a, **kw):
    return restate_row_form(*a, **kw) if form == "row" else restate_generic(*a, **kw)


def restate_teacher_lse(form, teacher, labels, vocab):
    """What ``ssi_ce_fwd(teacher, write_grad = 0)`` writes as row_lse (0 on a row without a valid label), by the restatement."""
    return restate(form, teacher, labels, vocab, mode("metrics"))["row_lse"]
