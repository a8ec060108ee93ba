"""GPU: ``ssi_edit_distance`` against the Python restatement (``tests/edit_ref.py``) and planted cases, exactly (integers: no tolerance).

The case table (``edit_ref.case_table``) pairs the lengths 0, 1, 2, C - 1, C, C + 1, 64 C - 1, 64 C, 64 C + 1 and one length inside the second
column block (C = ``_lib.EDIT_COLS``), the restatement capped at 300 a side and planted pairs above it; it runs once through the kernel form
for ``max_len > 64 C`` (column blocks, the boundary column in LDS) and, for its pairs that fit, once through the form for ``max_len <= 64 C``.
``ssi_edit_distance_workspace_bytes`` is 0 (nothing needs a workspace), so SSI_ERR_WORKSPACE cannot be provoked through a ``size_t``: what
is checked instead is that the size is 0 and that NULL is accepted."""
import ctypes

import pytest
import torch

import edit_ref
from ssi import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = _lib.EDIT_COLS
BLOCK = 64 * C
MAXLEN = _lib.EDIT_MAX_LEN


def pack(pairs, device=DEV):
    """Flat buffer and span arrays of ``(ref, hyp)`` pairs, every sequence stored once in order."""
    flat, rs, rl, hs, hl = [], [], [], [], []
    for ref, hyp in pairs:
        rs.append(len(flat)); rl.append(len(ref)); flat += ref
        hs.append(len(flat)); hl.append(len(hyp)); flat += hyp
    t = lambda v, dt: torch.tensor(v, dtype=dt, device=device)   # noqa: E731
    return t(flat, torch.int32), t(rs, torch.int64), t(rl, torch.int32), t(hs, torch.int64), t(hl, torch.int32)


def run(pairs, max_len):
    tokens, rs, rl, hs, hl = pack(pairs)
    out = torch.full((len(pairs), 4), -7, dtype=torch.int32, device=DEV)
    ops.edit_distance(tokens, rs, rl, hs, hl, out, max_len)
    return out.cpu().tolist()


@pytest.fixture(scope="module")
def table():
    cases = edit_ref.case_table(C)
    return cases, [edit_ref.expected(c) for c in cases]


def test_case_table_through_the_column_block_form(table):
    cases, want = table
    got = run([(c[1], c[2]) for c in cases], MAXLEN)
    bad = [(c[0], tuple(g), w) for c, g, w in zip(cases, got, want) if tuple(g) != w]
    assert not bad, bad[:10]


def test_case_table_through_the_single_block_form(table):
    cases, want = table
    keep = [k for k, c in enumerate(cases) if len(c[1]) <= BLOCK and len(c[2]) <= BLOCK]
    assert any(len(cases[k][2]) == BLOCK for k in keep)
    got = run([(cases[k][1], cases[k][2]) for k in keep], BLOCK)
    bad = [(cases[k][0], tuple(g), want[k]) for k, g in zip(keep, got) if tuple(g) != want[k]]
    assert not bad, bad[:10]


def test_invariants_hold_on_the_kernel_output(table):
    cases, _ = table
    pairs = [(c[1], c[2]) for c in cases] + [(c[2], c[1]) for c in cases]
    got = run(pairs, MAXLEN)
    n = len(cases)
    for k, ((ref, hyp), (dist, s, d, i)) in enumerate(zip(pairs, got)):
        assert dist == s + d + i and len(ref) - s - d == len(hyp) - s - i >= 0, (k, dist, s, d, i)
        assert got[(k + n) % (2 * n)][0] == dist                       # symmetric in the two arguments


def test_the_longest_pairs():
    ref, hyp, want = edit_ref.planted(MAXLEN, 26, 17, 17, seed=4096)
    hyp = hyp[:MAXLEN]
    assert len(ref) == MAXLEN and len(hyp) == MAXLEN                      # as many insertions as deletions
    one = [ref[1234]]
    got = run([(ref, hyp), (ref, one), (one, ref), (ref, [-5])], MAXLEN)
    assert tuple(got[0]) == want
    assert tuple(got[1]) == (MAXLEN - 1, 0, MAXLEN - 1, 0)                # one hit, the rest deleted
    assert tuple(got[2]) == (MAXLEN - 1, 0, 0, MAXLEN - 1)
    assert tuple(got[3]) == (MAXLEN, 1, MAXLEN - 1, 0)                    # no hit: one substitution (the diagonal comes first)


@pytest.mark.parametrize("max_len", [BLOCK, MAXLEN])
def test_bad_spans_give_minus_one_and_leave_their_neighbours_exact(max_len):
    rng = __import__("random").Random(5)
    seqs = [edit_ref.random_pair(rng, 30 + k, 25 + 2 * k, 3) for k in range(9)]
    tokens, rs, rl, hs, hl = pack(seqs)
    n_tokens = tokens.numel()
    want = [edit_ref.edit_counts(r, h) for r, h in seqs]
    rl[1] = max_len + 1                     # a length above max_len
    hl[2] = -1                              # a negative length
    rs[4] = -1                              # a negative start
    hs[5] = n_tokens + 1                    # a start beyond n_tokens
    rs[7] = n_tokens - 3                    # start + len beyond n_tokens
    bad = {1, 2, 4, 5, 7}
    out = torch.full((9, 4), -7, dtype=torch.int32, device=DEV)
    ops.edit_distance(tokens, rs, rl, hs, hl, out, max_len)
    got = out.cpu().tolist()
    for k in range(9):
        assert tuple(got[k]) == ((-1,) * 4 if k in bad else want[k]), (k, got[k])


def test_a_pair_is_bit_equal_wherever_it_lies():
    rng = __import__("random").Random(9)
    pair = edit_ref.random_pair(rng, 290, 300, 3)
    want = edit_ref.edit_counts(*pair)
    filler = [edit_ref.random_pair(rng, rng.randint(0, 40), rng.randint(0, 40), 2) for _ in range(1028)]
    alone = run([pair], MAXLEN)[0]
    first = run([pair] + filler[:4], MAXLEN)[0]
    late = run(filler[:1000] + [pair] + filler[1000:], MAXLEN)
    assert len(late) == 1029
    assert tuple(alone) == tuple(first) == tuple(late[1000]) == want


def test_overlapping_spans_and_one_span_twice():
    rng = __import__("random").Random(11)
    flat = [rng.randrange(4) for _ in range(400)]
    spans = [((0, 300), (100, 300)), ((50, 120), (50, 120)), ((399, 1), (0, 400)), ((200, 0), (200, 0)), ((10, 257), (9, 259))]
    t = lambda v, dt: torch.tensor(v, dtype=dt, device=DEV)   # noqa: E731
    out = torch.full((len(spans), 4), -7, dtype=torch.int32, device=DEV)
    ops.edit_distance(t(flat, torch.int32), t([a[0] for a, _ in spans], torch.int64), t([a[1] for a, _ in spans], torch.int32),
                      t([b[0] for _, b in spans], torch.int64), t([b[1] for _, b in spans], torch.int32), out, 400)
    got = out.cpu().tolist()
    for k, ((a0, al), (b0, bl)) in enumerate(spans):
        if max(al, bl) <= edit_ref.CAP:
            assert tuple(got[k]) == edit_ref.edit_counts(flat[a0:a0 + al], flat[b0:b0 + bl]), k
    assert tuple(got[1]) == (0, 0, 0, 0) and tuple(got[3]) == (0, 0, 0, 0)
    dist, s, d, i = got[2]                                                # 1 x 400 over an alphabet of 4: the id occurs, one hit
    assert (dist, s, d, i) == (399, 0, 0, 399)


def test_host_refusals_come_before_any_launch():
    lib = _lib.load()
    tokens, rs, rl, hs, hl = pack([([1, 2, 3], [1, 3])])
    out = torch.full((1, 4), -7, dtype=torch.int32, device=DEV)
    p = lambda x: ctypes.c_void_p(x.data_ptr())   # noqa: E731
    call = lambda **kw: lib.ssi_edit_distance(*[kw.get(k, v) for k, v in (   # noqa: E731
        ("tokens", p(tokens)), ("n_tokens", 5), ("rs", p(rs)), ("rl", p(rl)), ("hs", p(hs)), ("hl", p(hl)), ("n_pairs", 1), ("max_len", 16),
        ("out", p(out)), ("ws", None), ("ws_bytes", 0), ("stream", _lib.stream_ptr()))])
    ERR_ARG, ERR_UNSUPPORTED = 1, 2
    assert call(max_len=MAXLEN + 1) == ERR_UNSUPPORTED
    assert call(max_len=-1) == ERR_ARG and call(n_tokens=-1) == ERR_ARG and call(n_pairs=-1) == ERR_ARG
    assert call(n_pairs=2 ** 31) == ERR_ARG
    for name in ("tokens", "rs", "rl", "hs", "hl", "out"):
        assert call(**{name: None}) == ERR_ARG, name
    assert lib.ssi_edit_distance_workspace_bytes(1, 16) == 0 and lib.ssi_edit_distance_workspace_bytes(2 ** 31 - 1, MAXLEN) == 0
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [[-7] * 4]                               # nothing was launched
    assert call() == 0                                                     # the same call, unrefused (workspace NULL)
    assert out.cpu().tolist() == [[1, 0, 1, 0]]
    with pytest.raises(_lib.HipLibraryError):
        ops.edit_distance(tokens.cpu(), rs, rl, hs, hl, out, 16)


def test_no_pairs_launches_nothing():
    lib = _lib.load()
    assert lib.ssi_edit_distance(None, 0, None, None, None, None, 0, 16, None, None, 0, _lib.stream_ptr()) == 0
    e64, e32 = torch.empty(0, dtype=torch.int64, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV)
    ops.edit_distance(torch.zeros(4, dtype=torch.int32, device=DEV), e64, e32, e64, e32, torch.empty(0, 4, dtype=torch.int32, device=DEV), 16)
    torch.cuda.synchronize()
