"""The attention stress references and the per-row checker (tests/attn_stress.py) held against each other on the CPU, for every case and shape
that test_attn_stress_gpu.py runs: the share of rows in which the checker is blind stays under its cap; a second legitimate restatement of the
kernels' rounding passes with half the margin to spare; deliberately wrong results are flagged, at the row that was made wrong; and the global
criteria of the older parity tests accept a zeroed row, which is what the per-row tests add.  The same three properties for every (case,
geometry) of test_attn_generic_geometry_gpu.py (``attn_stress.GEOMETRIES``: head_dim 16, 32, 64 and 128, one, three and eight query heads per
kv head), with the planted errors at three query heads per kv head."""
import pytest
import torch

import attn_stress as A

CONFIGS = [(c, sh, None) for sh in A.SHAPES for c in A.CASES] + [(c, A.SHAPES[0], rows) for c, rows in A.DOC_CASES]
IDS = [f"{c}-{sh[0]}x{sh[1]}-{sh[2]}h{sh[3]}kv" + ("-docs" if rows else "") for c, sh, rows in CONFIGS]


def _refs(case, shape, rows):
    return A.exact(case, *shape, rows), A.restated(case, *shape, rows)


def _checks(got, ex, rs, shape, margin=A.MARGIN, hd=A.HD):
    """row_check of a full result dict (out + dqkv) against the references: {block: RowCheck}."""
    B, S, H, KV = shape
    res = {"out": A.row_check(got["out"], ex["out"], rs["out"], "out", B, S, margin=margin, hd=hd)}
    for block in A.BLOCKS:
        lo, hi = A.block_cols(block, H, KV, hd)
        res[block] = A.row_check(got["dqkv"][:, lo:hi], ex["dqkv"][:, lo:hi], rs["dqkv"][:, lo:hi], block, B, S, margin=margin,
                                 dq_cond=ex["dq_cond"] if block == "dq" else None, hd=hd)
    return res


def _seeded_row(check, seed):
    """A (batch row, position, head) drawn from the rows in which the checker is not blind (their share is capped separately)."""
    idx = torch.nonzero(~check.blind_rows)
    g = torch.Generator().manual_seed(seed)
    return tuple(int(i) for i in idx[int(torch.randint(len(idx), (1,), generator=g))])


@pytest.mark.parametrize("case,shape,rows", CONFIGS, ids=IDS)
def test_blind_share_and_second_restatement(case, shape, rows):
    """The blind share (rows with 16 E_row > max(|exact_row|, 0.02 rms_row)) is at most 6 % per block; the second restatement (P rounded
    un-normalised under a maximum stale by 3.7, O divided by l afterwards, delta from that O) stays within 4 E_row on every row — half the
    margin of 8 that the kernels get — and within the lse tolerance."""
    ex, rs = _refs(case, shape, rows)
    res = _checks(A.restated_second(case, *shape, rows), ex, rs, shape, margin=4.0)
    report = "; ".join(f"{b}: second restatement {c.worst:.2f} E_row, blind {100 * c.blind:.2f} %" for b, c in res.items())
    print(report)
    for block, c in res.items():
        assert c.blind <= A.BLIND_CAP, report
        assert c.ok, c.message + " | " + report
    for other in (rs, A.restated_second(case, *shape, rows)):
        err = float((other["lse"] - ex["lse"]).abs().max())
        assert err <= ex["lse_tol"], (err, ex["lse_tol"])
    assert 2e-5 <= ex["lse_tol"] <= 2e-4, ex["lse_tol"]   # (8 fp32 roundings of an lse of up to 67: the tolerance is computed, this is its sanity)


@pytest.mark.parametrize("case,shape,rows", CONFIGS, ids=IDS)
def test_checker_flags_a_zeroed_row(case, shape, rows):
    B, S, H, KV = shape
    ex, rs = _refs(case, shape, rows)
    clean = _checks(rs, ex, rs, shape)
    assert all(c.ok and c.worst <= 1.0 for c in clean.values())
    for block, nh, seed in (("dq", H, 11), ("dk", KV, 12)):
        b, s, h = _seeded_row(clean[block], seed)
        lo, _ = A.block_cols(block, H, KV)
        bad = {"out": rs["out"], "dqkv": rs["dqkv"].clone()}
        bad["dqkv"][b * S + s, lo + h * A.HD: lo + (h + 1) * A.HD] = 0
        c = _checks(bad, ex, rs, shape)[block]
        assert not c.ok and c.where == (b, s, h) and c.worst > 16.0, c.message
        assert int((c.ratio > A.MARGIN).sum()) == 1, c.message


@pytest.mark.parametrize("case,shape,rows", CONFIGS, ids=IDS)
def test_checker_flags_a_dropped_diagonal_key(case, shape, rows):
    """The last 64 queries of every batch row do not see their own key: flagged in out and in dv, in one of the last 64 rows, and no other row
    of out moves.  In ``fall`` the diagonal key holds the row's SMALLEST score.  At S = 512 (one document) it lies 7 to 8 below the first key's, a
    probability of about 1e-5: its loss moves nothing by a bf16 step, no test of the results could see it, and the wrong result must PASS.  At
    S = 256 and in the shorter documents it lies 1 to 6 below and at least one block must flag it."""
    B, S, H, KV = shape
    ex, rs = _refs(case, shape, rows)
    mask = A.dense_mask(B, S, rows)
    q = torch.arange(S - 64, S)
    mask[:, q, q] = False
    c = _checks(A.restate(case, *shape, rows, mask=mask), ex, rs, shape)
    flagged = [x for x in c.values() if not x.ok]
    assert all(x.where[1] >= S - 64 for x in flagged), [x.message for x in flagged]
    assert float(c["out"].ratio[:, : S - 64].max()) <= 1.0
    if case == "fall":
        assert bool(flagged) == (not (rows is None and S == 512)), [x.message for x in c.values()]
    else:
        assert not c["out"].ok and not c["dv"].ok, (c["out"].message, c["dv"].message)


@pytest.mark.parametrize("case,shape,rows", CONFIGS, ids=IDS)
def test_checker_flags_a_head_left_out_of_dk(case, shape, rows):
    B, S, H, KV = shape
    ex, rs = _refs(case, shape, rows)
    c = _checks(A.restate(case, *shape, rows, skip_dk_head=2), ex, rs, shape)
    assert not c["dk"].ok and c["dk"].where[2] == KV - 1, c["dk"].message
    assert KV == 1 or float(c["dk"].ratio[:, :, : KV - 1].max()) <= 1.0
    assert float((c["dk"].ratio[:, :, KV - 1] > A.MARGIN).double().mean()) > 0.5, c["dk"].message   # most rows of that head, not one outlier
    assert c["out"].ok and c["dq"].ok and c["dv"].ok


@pytest.mark.parametrize("shape", A.SHAPES, ids=[f"{s[0]}x{s[1]}" for s in A.SHAPES])
def test_the_global_criteria_accept_a_zeroed_row(shape):
    """What the per-row check adds, in code.  The criteria of the older fp32-SDPA tests are global: max|err| <= 3e-2 max|grad| over dqkv and a
    Frobenius ratio <= 1.5e-2 per block.  On ``gauss`` at these small shapes they accept the loss of a whole (row, head) of dq for 8-35 % of
    the rows and of a row of dk for 17-29 % (measured, with a little room left for the rounding of the other rows; asserted: at least 5 %; at the older tests' shapes, up to 500 k rows
    and max|grad| inflated by a x6 key, it is all of them).  One such row of each block, drawn by seed, is zeroed in a copy of the restated
    result: the global criteria pass it, row_check flags both rows and no other."""
    B, S, H, KV = shape
    ex, rs = _refs("gauss", shape, None)
    clean = _checks(rs, ex, rs, shape)
    want = ex["dqkv"]
    bad = rs["dqkv"].clone()
    rows_hit, share = {}, {}
    for block, seed in (("dq", 11), ("dk", 12)):
        lo, hi = A.block_cols(block, H, KV)
        w = want[:, lo:hi].view(B, S, -1, A.HD)
        unseen = (w.abs().amax(-1) <= 0.029 * float(want.abs().max())) & (w.norm(dim=-1) <= 0.012 * float(want[:, lo:hi].norm()))
        share[block] = float(unseen.double().mean())
        idx = torch.nonzero(unseen & ~clean[block].blind_rows)
        b, s, h = rows_hit[block] = tuple(int(i) for i in idx[int(torch.randint(len(idx), (1,), generator=torch.Generator().manual_seed(seed)))])
        bad[b * S + s, lo + h * A.HD: lo + (h + 1) * A.HD] = 0
    mx = float((bad - want).abs().max()) / float(want.abs().max())
    fro = {}
    for block in A.BLOCKS:
        lo, hi = A.block_cols(block, H, KV)
        fro[block] = float((bad[:, lo:hi] - want[:, lo:hi]).norm() / want[:, lo:hi].norm())
    report = (f"share of rows whose loss the global criteria accept {share}; zeroed {rows_hit}: max|err| / max|grad| {mx:.4f} (limit 0.03), "
              f"Frobenius ratios {fro} (limit 0.015)")
    print(report)
    assert min(share.values()) >= 0.05, report
    assert mx <= 3e-2 and all(v <= 1.5e-2 for v in fro.values()), report
    c = _checks({"out": rs["out"], "dqkv": bad}, ex, rs, shape)
    for block in ("dq", "dk"):
        assert not c[block].ok and c[block].where == rows_hit[block] and int((c[block].ratio > A.MARGIN).sum()) == 1, c[block].message
    assert c["dv"].ok


# ---- the head geometries of the generic kernels (attn_stress.GEOMETRIES) ---------------------------------------------------------------
@pytest.mark.parametrize("hd,shape,rows,case", A.GEO_CONFIGS, ids=A.GEO_IDS)
def test_geometry_blind_share_and_second_restatement(hd, shape, rows, case):
    """As ``test_blind_share_and_second_restatement``, at every head_dim and head ratio the generic kernels are tested at: blind share at most
    ``BLIND_CAP`` per block (what decides which cases a geometry gets: ``sink`` is over it on the short rows and is not in their lists), the
    second restatement within 4 E_row — half of ``MARGIN`` — on every row (measured: at most 3.54, dk in ``sharp`` at head_dim 128), lse of
    both restatements within its tolerance."""
    ex, rs = A.exact(case, *shape, rows, hd=hd), A.restated(case, *shape, rows, hd=hd)
    second = A.restated_second(case, *shape, rows, hd=hd)
    res = _checks(second, ex, rs, shape, margin=4.0, hd=hd)
    report = "; ".join(f"{b}: second restatement {c.worst:.2f} E_row, blind {100 * c.blind:.2f} %" for b, c in res.items())
    print(report)
    for block, c in res.items():
        assert c.blind <= A.BLIND_CAP, report
        assert c.ok and c.worst <= A.MARGIN, c.message + " | " + report
    for other in (rs, second):
        err = float((other["lse"] - ex["lse"]).abs().max())
        assert err <= ex["lse_tol"], (err, ex["lse_tol"])
    assert 2e-5 <= ex["lse_tol"] <= 2e-4, ex["lse_tol"]
    # the fp32 forms (restated = the exact result rounded to fp32, eps = EPS_F32): no blind row at all
    f32 = A.f32_restated(ex)
    B, S, H, KV = shape
    for block in A.BLOCKS:
        lo, hi = A.block_cols(block, H, KV, hd)
        c = A.row_check(f32["dqkv"][:, lo:hi], ex["dqkv"][:, lo:hi], f32["dqkv"][:, lo:hi], block, B, S, eps=A.EPS_F32,
                        dq_cond=ex["dq_cond"] if block == "dq" else None, hd=hd)
        assert c.blind == 0.0 and c.worst <= 1.0, c.message


def test_sink_is_over_the_cap_on_the_short_rows():
    """Why ``sink`` is not in the short geometries' case lists: the reference alone is blind on more than ``BLIND_CAP`` of the dq rows there
    (8.5 - 18 %), and on 5.8 % at the 3B shape, where it is kept."""
    for hd, shape, rows, cases in A.GEOMETRIES:
        if rows is not None or len(cases) == 1:      # (the lists that name their few cases; the others take every case the cap allows)
            continue
        ex, rs = A.exact("sink", *shape, hd=hd), A.restated("sink", *shape, hd=hd)
        blind = _checks(rs, ex, rs, shape, hd=hd)["dq"].blind
        print(f"hd {hd} {shape}: sink dq blind share {100 * blind:.1f} %")
        assert ("sink" in cases) == (blind <= A.BLIND_CAP), (hd, shape, blind)


REP3 = [(128, A.GEO_3B), (16, (2, 130, 3, 1))]
REP3_IDS = ["hd128-6h2kv", "hd16-3h1kv"]


@pytest.mark.parametrize("case", ("gauss", "ramp8", "fall", "sharp"))
@pytest.mark.parametrize("hd,shape", REP3, ids=REP3_IDS)
def test_checker_flags_each_head_of_a_group_of_three_left_out_of_dk(hd, shape, case):
    """Three query heads per kv head (``e / rep``, ``e % rep`` in the generic dK/dV kernel): each of the three left out of dk of the last kv
    head is flagged, on most rows of that head and on no row of another, and out, dq and dv stay clean."""
    B, S, H, KV = shape
    assert H // KV == 3
    ex, rs = A.exact(case, *shape, hd=hd), A.restated(case, *shape, hd=hd)
    for head in range(3):
        c = _checks(A.restate(case, *shape, hd=hd, skip_dk_head=head), ex, rs, shape, hd=hd)
        assert not c["dk"].ok and c["dk"].where[2] == KV - 1, c["dk"].message
        assert KV == 1 or float(c["dk"].ratio[:, :, : KV - 1].max()) <= 1.0
        assert float((c["dk"].ratio[:, :, KV - 1] > A.MARGIN).double().mean()) > 0.5, c["dk"].message
        assert c["out"].ok and c["dq"].ok and c["dv"].ok


@pytest.mark.parametrize("case", ("gauss", "ramp8", "fall", "sharp"))
@pytest.mark.parametrize("hd,shape", REP3, ids=REP3_IDS)
def test_checker_flags_a_wrong_mask_at_three_heads_per_kv_head(hd, shape, case):
    """The last 64 queries of every batch row do not see their own key: out and dv are flagged, in one of those rows, and no other row of out
    moves (rows this short leave the diagonal key of ``fall`` a visible share too)."""
    B, S, H, KV = shape
    ex, rs = A.exact(case, *shape, hd=hd), A.restated(case, *shape, hd=hd)
    mask = A.dense_mask(B, S)
    q = torch.arange(S - 64, S)
    mask[:, q, q] = False
    c = _checks(A.restate(case, *shape, hd=hd, mask=mask), ex, rs, shape, hd=hd)
    assert not c["out"].ok and not c["dv"].ok, (c["out"].message, c["dv"].message)
    assert all(x.where[1] >= S - 64 for x in c.values() if not x.ok)
    assert float(c["out"].ratio[:, : S - 64].max()) <= 1.0
