"""The attention stress references and the per-row checker (tests/attn_stress.py) held against each other on the CPU, for every case and shape
that test_attn_stress_gpu.py runs: the share of rows in which the checker is blind stays under its cap; a second legitimate restatement of the
kernels' rounding passes with half the margin to spare; deliberately wrong results are flagged, at the row that was made wrong; and the global
criteria of the older parity tests accept a zeroed row, which is what the per-row tests add."""
import pytest
import torch

import attn_stress as A

CONFIGS = [(c, sh, None) for sh in A.SHAPES for c in A.CASES] + [(c, A.SHAPES[0], rows) for c, rows in A.DOC_CASES]
IDS = [f"{c}-{sh[0]}x{sh[1]}-{sh[2]}h{sh[3]}kv" + ("-docs" if rows else "") for c, sh, rows in CONFIGS]


def _refs(case, shape, rows):
    return A.exact(case, *shape, rows), A.restated(case, *shape, rows)


def _checks(got, ex, rs, shape, margin=A.MARGIN):
    """row_check of a full result dict (out + dqkv) against the references: {block: RowCheck}."""
    B, S, H, KV = shape
    res = {"out": A.row_check(got["out"], ex["out"], rs["out"], "out", B, S, margin=margin)}
    for block in A.BLOCKS:
        lo, hi = A.block_cols(block, H, KV)
        res[block] = A.row_check(got["dqkv"][:, lo:hi], ex["dqkv"][:, lo:hi], rs["dqkv"][:, lo:hi], block, B, S, margin=margin,
                                 dq_cond=ex["dq_cond"] if block == "dq" else None)
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
