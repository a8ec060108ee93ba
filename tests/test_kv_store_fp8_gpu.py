"""``ssi_kv_store_fp8`` on the GPU: the codes and exponent bytes of every stored line are EXACTLY those of kv_fp8_ref.py, for bf16 and fp32 rows.

Geometries (n_kv, head_dim) = (2, 16), (1, 64), (8, 64), (1, 128) — one to sixteen lanes a line (and head_dim 24: lanes of a line idle) — with 1, 5 and
300 rows (more than one workgroup).  The lines of a launch cycle through ``kv_fp8_ref.edge_lines`` — all zeros; an absmax with mantissa exactly 1.75
and one ulp either side; absmax = 448 * 2^k; elements on e4m3 midpoints of both parities; elements among the e4m3 subnormals, at and around half the
smallest; a NaN and infinities; nothing finite; large, tiny and subnormal magnitudes — with drawn lines of mixed magnitude between them, so K and V
lines and neighbouring heads differ in exponent.  Rows go to a permutation of the cache's positions; ``dest = -1`` skips a row, a ``dest`` outside the
cache is counted once and writes nothing, and every byte no ``dest`` names still holds its sentinel."""
import pytest
import torch

import kv_fp8_ref as kr

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTYPES = (torch.bfloat16, torch.float32)
GEOMS = ((2, 16), (1, 64), (8, 64), (1, 128), (3, 24))
SENTINEL = 0xA5


def _name(dt):
    return "bf16" if dt == torch.bfloat16 else "fp32"


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


def make_rows(n_kv, hd, dtype, rows, seed=7):
    """qkv [rows, ld] (two query heads per kv head, 8 pad columns) whose k and v lines cycle through the edge lines and drawn ones."""
    g = torch.Generator().manual_seed(seed)
    edges = kr.edge_lines(hd, dtype)
    n_lines = rows * 2 * n_kv
    drawn = (torch.randn(n_lines, hd, generator=g) * torch.exp2(torch.randint(-12, 12, (n_lines, 1), generator=g).float())).to(dtype)
    lines = drawn.clone()
    take = torch.arange(n_lines) % 3 != 2                               # two of three lines an edge line, shifted so K, V and heads see all of them
    idx = (torch.arange(n_lines) * 7 + 3) % edges.shape[0]
    lines[take] = edges[idx[take]]
    H = 2 * n_kv
    qkv = torch.randn(rows, (H + 2 * n_kv) * hd + 8, generator=g).to(dtype)
    qkv[:, H * hd:(H + 2 * n_kv) * hd] = lines.view(rows, 2 * n_kv * hd)
    return qkv, H


def run(ops, qkv, dest, n_slots, cap, H, n_kv, hd):
    kc, vc = (torch.full((n_slots, cap, n_kv * hd), SENTINEL, dtype=torch.uint8, device=DEV) for _ in range(2))
    ke, ve = (torch.full((n_slots, cap, n_kv), SENTINEL, dtype=torch.uint8, device=DEV) for _ in range(2))
    n_bad = torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.kv_store_fp8(qkv.to(DEV), dest.to(DEV), kc, vc, ke, ve, H, n_kv, hd, n_bad=n_bad)
    torch.cuda.synchronize()
    return kc.cpu(), vc.cpu(), ke.cpu(), ve.cpu(), int(n_bad)


def expected(qkv, dest, n_slots, cap, H, n_kv, hd):
    rows = qkv.shape[0]
    kv = qkv[:, H * hd:(H + 2 * n_kv) * hd].view(rows, 2, n_kv, hd)
    codes, b = kr.quantise(kv)
    out = [torch.full((n_slots * cap, n_kv * hd), SENTINEL, dtype=torch.uint8) for _ in range(2)]
    out += [torch.full((n_slots * cap, n_kv), SENTINEL, dtype=torch.uint8) for _ in range(2)]
    ok = (dest >= 0) & (dest < n_slots * cap)
    for which in (0, 1):
        out[which][dest[ok]] = codes[ok, which].reshape(-1, n_kv * hd)
        out[2 + which][dest[ok]] = b[ok, which]
    bad = int(((dest != -1) & ~ok).sum())
    return [t.view(n_slots, cap, -1) for t in out], bad


def describe(got, want, name):
    d = (got != want).nonzero()
    return f"{name}: {d.shape[0]} bytes differ, first at {d[0].tolist()}: got {int(got[tuple(d[0])]):#x}, expected {int(want[tuple(d[0])]):#x}" if d.numel() else ""


@pytest.mark.parametrize("rows", (1, 5, 300))
@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
@pytest.mark.parametrize("geom", GEOMS, ids=lambda g: f"{g[0]}kv{g[1]}")
def test_codes_and_exponents_are_exactly_the_references(ops, geom, dtype, rows):
    n_kv, hd = geom
    qkv, H = make_rows(n_kv, hd, dtype, rows)
    n_slots, cap = 3, (rows + 2) // 3 + 2                               # more positions than rows: some keep their sentinel
    g = torch.Generator().manual_seed(rows)
    dest = torch.randperm(n_slots * cap, generator=g)[:rows].to(torch.int64)
    if rows >= 5:
        dest[1] = -1                                                    # skipped ...
        dest[3] = n_slots * cap                                         # ... and refused: one past the end, far out, negative
    if rows == 300:
        dest[100], dest[299], dest[7] = 1 << 40, -2, -1
    got = run(ops, qkv, dest, n_slots, cap, H, n_kv, hd)
    want, bad = expected(qkv, dest, n_slots, cap, H, n_kv, hd)
    msgs = [describe(a, b, n) for a, b, n in zip(got[:4], want, ("k_codes", "v_codes", "k_exp", "v_exp"))]
    assert not any(msgs), msgs
    assert got[4] == bad
    untouched = torch.ones(n_slots * cap, dtype=torch.bool)
    untouched[dest[(dest >= 0) & (dest < n_slots * cap)]] = False
    assert int(untouched.sum()) >= 2
    for t in got[:4]:                                                   # (implied by the comparison; said once more on its own)
        assert bool((t.view(n_slots * cap, -1)[untouched] == SENTINEL).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=_name)
def test_every_edge_line_on_its_own(ops, dtype):
    """One line a row, K and V the same line, so a failure names the class of input."""
    n_kv, hd = 1, 64
    edges = kr.edge_lines(hd, dtype)
    rows, H = edges.shape[0], 1
    qkv = torch.zeros(rows, 3 * hd, dtype=dtype)
    qkv[:, hd:2 * hd], qkv[:, 2 * hd:] = edges, edges
    dest = torch.arange(rows, dtype=torch.int64)
    got = run(ops, qkv, dest, 1, rows, H, n_kv, hd)
    want, _ = expected(qkv, dest, 1, rows, H, n_kv, hd)
    wrong = [kr.EDGE_NAMES[r] for r in range(rows)
             if not all(torch.equal(a[0, r], b[0, r]) for a, b in zip(got[:4], want))]
    assert wrong == [], [(n, got[0][0, kr.EDGE_NAMES.index(n)][:16].tolist(), want[0][0, kr.EDGE_NAMES.index(n)][:16].tolist(),
                          int(got[2][0, kr.EDGE_NAMES.index(n)]), int(want[2][0, kr.EDGE_NAMES.index(n)])) for n in wrong]
    assert torch.equal(got[0], got[1]) and torch.equal(got[2], got[3])


def test_all_rows_skipped_or_refused_write_nothing(ops):
    n_kv, hd = 2, 16
    qkv, H = make_rows(n_kv, hd, torch.bfloat16, 6)
    dest = torch.tensor([-1, 24, -5, -1, 1 << 35, -1], dtype=torch.int64)
    got = run(ops, qkv, dest, 2, 12, H, n_kv, hd)
    assert got[4] == 3
    for t in got[:4]:
        assert bool((t == SENTINEL).all())
