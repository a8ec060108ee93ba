"""Python restatement of the edit distance of ``include/ssi_hip.h`` (``ssi_edit_distance``), a builder of planted cases whose answer needs no
dynamic programme, and the case table of the GPU test.

THE DEFINITION, restated.  For a reference ``r[0..m)`` and a hypothesis ``h[0..n)`` of int32 ids, compared by equality only, the cell
``(i, j)`` holds ``(cost, S, D, I)``.  Row 0 is ``(j, 0, 0, j)``; column 0 is ``(i, 0, i, 0)``.  For ``i, j >= 1`` there are three candidates,
taken in this order, a later one replacing an earlier one only on strictly lower cost: 1. the diagonal, ``+ 0`` if ``r[i-1] == h[j-1]`` else
``+ 1`` cost and ``+ 1`` S; 2. up, from ``(i-1, j)``, ``+ 1`` cost and ``+ 1`` D; 3. left, from ``(i, j-1)``, ``+ 1`` cost and ``+ 1`` I.
The result is the cell ``(m, n)`` as ``(dist, S, D, I)``."""
import random

CAP = 300          # the restatement is quadratic in Python: pairs with a side above this are checked by planted cases only
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
# switches of ``edit_counts`` that plant one defect each (``test_edit_ref`` shows that the case table catches every one)
DEFECTS = ("tie_order", "le_for_lt", "boundary_swapped", "s_on_hit", "d_i_exchanged")


def edit_counts(r, h, defect=None):
    """``(dist, S, D, I)`` of the definition; ``defect`` plants one of ``DEFECTS``."""
    assert defect is None or defect in DEFECTS
    m, n = len(r), len(h)
    swapped = defect == "boundary_swapped"
    lower = (lambda a, b: a <= b) if defect == "le_for_lt" else (lambda a, b: a < b)
    prev = [(j, 0, j, 0) if swapped else (j, 0, 0, j) for j in range(n + 1)]
    for i in range(1, m + 1):
        cur = [(i, 0, 0, i) if swapped else (i, 0, i, 0)]
        for j in range(1, n + 1):
            d, u, l = prev[j - 1], prev[j], cur[j - 1]
            hit = r[i - 1] == h[j - 1]
            diag = (d[0] + (0 if hit else 1), d[1] + (1 if (not hit or defect == "s_on_hit") else 0), d[2], d[3])
            up = (u[0] + 1, u[1], u[2], u[3] + 1) if defect == "d_i_exchanged" else (u[0] + 1, u[1], u[2] + 1, u[3])
            left = (l[0] + 1, l[1], l[2] + 1, l[3]) if defect == "d_i_exchanged" else (l[0] + 1, l[1], l[2], l[3] + 1)
            order = (left, up, diag) if defect == "tie_order" else (diag, up, left)
            best = order[0]
            for cand in order[1:]:
                if lower(cand[0], best[0]):
                    best = cand
            cur.append(best)
        prev = cur
    return prev[n]


def planted(m, n_sub, n_del, n_ins, seed, first_id=0, fresh_id=1 << 20):
    """``(ref, hyp, (dist, S, D, I))``: a reference of ``m`` distinct ids and a hypothesis made from it by ``n_sub`` single substitutions,
    ``n_del`` deletions and ``n_ins`` insertions (of fresh ids, each before a kept reference id), at least two untouched ids apart and
    away from both ends.  The optimal alignment is then unique, so the answer is the planted counts."""
    k = n_sub + n_del + n_ins
    slots = list(range(3, m - 3, 3))
    assert k <= len(slots), f"{k} edits do not fit {m} ids three apart"
    rng = random.Random(seed)
    where = rng.sample(slots, k)
    kinds = dict(zip(where, "S" * n_sub + "D" * n_del + "I" * n_ins))
    ref = [first_id + p for p in range(m)]
    hyp, fresh = [], fresh_id
    for p, t in enumerate(ref):
        kind = kinds.get(p)
        if kind == "S":
            hyp.append(fresh)
            fresh += 1
        elif kind == "I":
            hyp += [fresh, t]
            fresh += 1
        elif kind is None:
            hyp.append(t)
    return ref, hyp, (k, n_sub, n_del, n_ins)


def planted_to_lengths(m, n, seed):
    """A planted case with ``len(ref) == m`` and ``len(hyp) == n``: ``|m - n|`` deletions or insertions, and as many substitutions and
    deletion-insertion pairs beside them as fit, up to 5 each.  For ``n > m`` the case is planted the other way round and its two sides
    exchanged (a unique alignment read backwards: deletions become insertions)."""
    if n > m:
        hyp, ref, (k, s, i, d) = planted_to_lengths(n, m, seed)
        return ref, hyp, (k, s, d, i)
    room = len(range(3, m - 3, 3)) - (m - n)
    assert room >= 0, (m, n)
    extra = min(5, room // 3)
    return planted(m, extra, m - n + extra, extra, seed)


def disjoint(m, n):
    """``(ref, hyp, (dist, S, D, I))`` of two sequences with no id in common."""
    s = min(m, n)
    return list(range(m)), list(range(10 ** 6, 10 ** 6 + n)), (max(m, n), s, m - s, n - s)


def random_pair(rng, m, n, alphabet):
    return [rng.randrange(alphabet) for _ in range(m)], [rng.randrange(alphabet) for _ in range(n)]


def case_table(cols):
    """The pairs the GPU test runs, as ``(name, ref, hyp, expected or None)``; ``expected`` is set where the pair is planted (no dynamic
    programme), None where the restatement gives it.  ``cols`` is the kernel's columns per lane (``_lib.EDIT_COLS``): the lengths are those
    at which the kernel takes another path — 0, 1, 2, around one lane's strip, around one column block of ``64 * cols``, and one length
    inside the second block."""
    block = 64 * cols
    lengths = [0, 1, 2, cols - 1, cols, cols + 1, block - 1, block, block + 1, block + block // 2 + 3]
    lengths = sorted(set(lengths))
    rng = random.Random(20290)
    cases = []
    for m in lengths:
        for n in lengths:
            if m <= CAP and n <= CAP:
                for alphabet in (2, 50):
                    cases.append((f"random[{m}x{n},a{alphabet}]", *random_pair(rng, m, n, alphabet), None))
            elif len(range(3, max(m, n) - 3, 3)) >= abs(m - n):
                ref, hyp, want = planted_to_lengths(m, n, seed=m * 10007 + n)
                assert (len(ref), len(hyp)) == (m, n)
                cases.append((f"planted[{m}x{n}]", ref, hyp, want))
            else:
                # too unequal to plant (the edits would not fit two apart): disjoint ids.  Every cell of the table is a miss, so the answer
                # follows from the definition without a dynamic programme: cost(i, j) = max(i, j), the diagonal wins every tie it is in,
                # hence min(m, n) substitutions and |m - n| deletions or insertions (checked against the restatement in test_edit_ref)
                cases.append((f"disjoint[{m}x{n}]", *disjoint(m, n)))
    # alphabets: extreme ids, equal and disjoint sequences
    ext = [INT32_MIN, -1, INT32_MAX]
    cases.append(("extreme-ids", [ext[rng.randrange(3)] for _ in range(37)], [ext[rng.randrange(3)] for _ in range(41)], None))
    cases.append(("extreme-ids-planted", [INT32_MIN, -1, INT32_MAX, 0, 1], [INT32_MIN, -1, INT32_MAX - 1, 0, 1], (1, 1, 0, 0)))
    same = [rng.randrange(50) for _ in range(block + 7)]
    cases.append(("equal", same, list(same), (0, 0, 0, 0)))
    cases.append(("disjoint-short", list(range(0, 23)), list(range(100, 129)), None))
    # ties: the order of the three candidates and the strictness of the comparison decide these
    cases.append(("tie-sub-vs-del-ins", [1, 2], [2, 3], None))
    cases.append(("tie-one-id", [7], [8], None))
    cases.append(("tie-shift", [1, 2, 3, 4, 5, 6], [2, 3, 4, 5, 6, 7], None))
    cases.append(("tie-hit-late", [1, 1, 2], [1, 2], None))
    cases.append(("tie-hit-early", [1, 2], [1, 1, 2], None))
    return cases


def expected(case):
    name, ref, hyp, want = case
    return tuple(want) if want is not None else edit_counts(ref, hyp)


def mbr_ref(candidates):
    """The minimum-Bayes-risk order of one prompt's candidates (lists of ids), restated: ``risk_k`` is the mean over the other candidates
    ``c_j`` of ``dist(c_j, c_k) / max(1, len(c_j))`` in float64, summed in index order; the order is by rising risk, then index.
    Returns ``(order, risks)`` with ``risks`` indexed by candidate."""
    n = len(candidates)
    dist = [[edit_counts(candidates[j], candidates[k])[0] for k in range(n)] for j in range(n)]
    risks = []
    for k in range(n):
        total = 0.0
        for j in range(n):
            if j != k:
                total += dist[j][k] / max(1, len(candidates[j]))
        risks.append(total / (n - 1))
    return sorted(range(n), key=lambda k: (risks[k], k)), risks
