"""CPU: the Python restatement of the edit distance (``tests/edit_ref.py``) against the properties that follow from the definition, the
planted-case builder against the restatement, and the case table of the GPU test against five planted defects of the restatement."""
import random

import pytest

import edit_ref
from edit_ref import DEFECTS, case_table, disjoint, edit_counts, expected, planted, planted_to_lengths

COLS = 4   # any strip width gives a table with the small and the tie cases; the GPU test passes the kernel's


def test_invariants_on_random_pairs():
    rng = random.Random(1)
    for alphabet in (2, 3, 50):
        for _ in range(120):
            m, n = rng.randint(0, 20), rng.randint(0, 20)
            r, h = edit_ref.random_pair(rng, m, n, alphabet)
            c, s, d, i = edit_counts(r, h)
            assert c == s + d + i, (r, h)
            assert m - s - d == n - s - i >= 0, (r, h)
            assert edit_counts(h, r)[0] == c, (r, h)


def test_the_counts_are_not_symmetric():
    assert edit_counts([1, 2, 3], [1, 3]) == (1, 0, 1, 0) and edit_counts([1, 3], [1, 2, 3]) == (1, 0, 0, 1)


def test_hand_cases():
    assert edit_counts([], []) == (0, 0, 0, 0)
    assert edit_counts([5, 6], []) == (2, 0, 2, 0) and edit_counts([], [5, 6, 7]) == (3, 0, 0, 3)
    assert edit_counts([1, 2, 3, 4], [1, 9, 3, 4]) == (1, 1, 0, 0)
    assert edit_counts([1, 2], [2, 3]) == (2, 2, 0, 0)          # the diagonal is taken first and a tie does not replace it


@pytest.mark.parametrize("m,s,d,i", [(12, 1, 0, 0), (12, 0, 1, 0), (12, 0, 0, 1), (40, 3, 3, 3), (120, 9, 7, 11), (300, 26, 17, 17)])
def test_planted_cases_against_the_restatement(m, s, d, i):
    for seed in range(3):
        ref, hyp, want = planted(m, s, d, i, seed)
        assert len(ref) == m and len(hyp) == m - d + i and want == (s + d + i, s, d, i)
        assert edit_counts(ref, hyp) == want


@pytest.mark.parametrize("m,n", [(255, 256), (256, 255), (257, 257), (300, 290), (270, 300), (50, 37), (37, 50)])
def test_planted_to_lengths_against_the_restatement(m, n):
    ref, hyp, want = planted_to_lengths(m, n, seed=m + n)
    assert (len(ref), len(hyp)) == (m, n) and edit_counts(ref, hyp) == want


def test_disjoint_answer_against_the_restatement():
    for m in range(0, 14):
        for n in range(0, 14):
            ref, hyp, want = disjoint(m, n)
            assert edit_counts(ref, hyp) == want, (m, n)
    ref, hyp, want = disjoint(5, 290)
    assert edit_counts(ref, hyp) == want


def test_case_table_covers_what_the_issue_lists():
    cases = case_table(COLS)
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names)
    lengths = {0, 1, 2, COLS - 1, COLS, COLS + 1, 64 * COLS - 1, 64 * COLS, 64 * COLS + 1}
    seen = {(len(c[1]), len(c[2])) for c in cases}
    assert {(m, n) for m in lengths for n in lengths} <= seen
    assert any(m > 64 * COLS + 1 and n > 64 * COLS + 1 for m, n in seen)       # a pair inside the second column block
    for name, ref, hyp, want in cases:
        assert (want is None) == (len(ref) <= edit_ref.CAP and len(hyp) <= edit_ref.CAP and not name.endswith("planted") and name != "equal"), name
        assert all(edit_ref.INT32_MIN <= t <= edit_ref.INT32_MAX for t in ref + hyp)


@pytest.mark.parametrize("defect", DEFECTS)
def test_each_planted_defect_is_caught_by_the_case_table(defect):
    assert len(DEFECTS) >= 5
    small = [c for c in case_table(COLS) if len(c[1]) <= 40 and len(c[2]) <= 45]
    caught = [c[0] for c in small if edit_counts(c[1], c[2], defect) != expected(c)]
    assert caught, f"no case of the table catches {defect}"
