"""CPU: ``GroupClip`` (``ssi/grad_groups.py``, torch fp32 on CPU tensors) against the numpy restatement of the clip rule
(``tests/grad_groups_ref.py``) over a 12-step norm sequence with a spike, a zero norm, a NaN norm and the end of the warm-up, within 1e-6
relative (under ten fp32 operations of half an ulp each: 6e-7); and every planted defect of the restatement's mirror is caught by that bound."""
import math

import numpy as np
import pytest
import torch

import grad_groups_ref as ref

TOL = 1e-6
ADAPTIVE = {"rel": 1.05, "beta": 0.98, "warmup_steps": 4}
# steps:   1    2    3     4    5 (first after warm-up)  6 spike  7    8 zero  9 NaN  10   11 spike  12
NORMS = [2.0, 1.5, 0.0, 1.8, 1.7,                      40.0,    1.6, 0.0,    math.nan, 1.55, 9.0,    1.5]
# a second group: its first norms are zero and NaN (gamma stays unset past the warm-up), its threshold binds after the warm-up
NORMS_B = [0.0, math.nan, 0.0, 0.0, 0.0, 3.0, 2.5, 2.6, math.inf, 2.4, 2.7, 2.5]
MAX_B = 2.0


def _group_clip(max_norms, adaptive):
    from ssi.grad_groups import GroupClip
    return GroupClip([f"g{k}" for k in range(len(max_norms))], max_norms, adaptive)


def _run_torch(seqs, max_norms, adaptive, with_scale=False):
    clip = _group_clip(max_norms, adaptive)
    rows = []
    for t in range(len(seqs[0])):
        n = torch.tensor([s[t] for s in seqs], dtype=torch.float32)
        # the sums of squares and the pending scale the optimizer hands over: n = sqrt(sumsq) * |scale|
        scale = torch.tensor([-0.5]) if with_scale else None
        sumsq = (n / 0.5) ** 2 if with_scale else n ** 2
        c = clip.update(sumsq, scale)
        gamma = torch.where(clip.has_gamma > 0, clip.gamma, torch.full_like(clip.gamma, math.nan))
        rows.append(torch.stack([c, gamma, clip.skipped], dim=1).double().numpy())
    return np.stack(rows), clip          # [steps, groups, 3]


def _close(got, want):
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return bool(np.all(np.abs(got[ok] - want[ok]) <= TOL * np.abs(want[ok])))


@pytest.mark.parametrize("with_scale", [False, True])
def test_adaptive_equals_the_restatement(with_scale):
    got, clip = _run_torch([NORMS, NORMS_B], [math.inf, MAX_B], ADAPTIVE, with_scale)
    want = np.stack([ref.run(NORMS, adaptive=ADAPTIVE), ref.run(NORMS_B, max_norm=MAX_B, adaptive=ADAPTIVE)], axis=1)
    assert _close(got, want), (got, want)
    assert clip.t == 12
    # the sequence does what it is there for: the spikes are clipped, the skips counted, a zero norm leaves gamma alone, the threshold binds
    assert want[5, 0, 0] < 0.1 and want[10, 0, 0] < 0.3 and math.isnan(want[8, 0, 0]) and want[-1, 0, 2] == 1 and want[-1, 1, 2] == 2
    assert want[2, 0, 1] == want[1, 0, 1] and math.isnan(want[4, 1, 1]) and want[5, 1, 0] < 1


def test_fixed_mode_equals_the_restatement():
    got, _ = _run_torch([NORMS, NORMS_B], [1.0, math.inf], None)
    want = np.stack([ref.run(NORMS, max_norm=1.0), ref.run(NORMS_B)], axis=1)
    assert _close(got, want)
    assert np.all(np.isnan(want[:, :, 1]))                       # fixed mode keeps no average
    ok = ~np.isnan(want[:, 1, 0])
    assert np.all(want[ok, 1, 0] == 1.0)                         # a group that is never clipped: the coefficient is exactly 1


@pytest.mark.parametrize("defect", ref.DEFECTS)
def test_every_planted_defect_is_caught(defect):
    got, _ = _run_torch([NORMS, NORMS_B], [math.inf, MAX_B], ADAPTIVE)
    mirror = np.stack([ref.run(NORMS, adaptive=ADAPTIVE, defect=defect), ref.run(NORMS_B, max_norm=MAX_B, adaptive=ADAPTIVE, defect=defect)], axis=1)
    assert not _close(got, mirror), defect


def test_the_defect_list_covers_the_six_of_the_issue():
    assert len(ref.DEFECTS) >= 6 and len(set(ref.DEFECTS)) == len(ref.DEFECTS)


def test_state_dict_round_trip_and_a_group_without_state():
    got, clip = _run_torch([NORMS[:7], NORMS_B[:7]], [math.inf, MAX_B], ADAPTIVE)
    state = clip.state_dict()
    assert state["t"] == 7 and sorted(state["groups"]) == ["g0", "g1"]
    other = _group_clip([math.inf, MAX_B, 3.0], ADAPTIVE)       # one more group than was saved: it starts unset
    other.load_state_dict(state)
    assert other.t == 7 and float(other.has_gamma[2]) == 0 and torch.equal(other.gamma[:2], clip.gamma) and torch.equal(other.skipped[:2], clip.skipped)
    for t in range(7, 12):                                      # the resumed rule continues bit for bit
        n = torch.tensor([NORMS[t], NORMS_B[t]], dtype=torch.float32)
        a = clip.update(n ** 2, None)
        b = other.update(torch.cat([n, torch.tensor([1.0])]) ** 2, None)
        assert torch.equal(a.view(torch.int32), b[:2].view(torch.int32))
    assert torch.equal(other.gamma[:2], clip.gamma)
