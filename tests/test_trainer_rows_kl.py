"""CPU: the KL part of the objective (``kl_loss``, ``teacher_kl_coeff``) in the trainer's by-name records — the read-back row of a micro-batch
and the window's data-parallel scalars round-trip with it alone and with every part in the trainer's order; off by default."""
import torch


def test_the_part_is_listed_after_the_two_of_before_and_off_by_default():
    from ssi.trainer import AUX_PARTS, TEACHER_PARTS, Trainer
    assert TEACHER_PARTS == (("kl_loss", "teacher_kl_coeff"),)
    assert [name for name, _ in AUX_PARTS + TEACHER_PARTS] == ["z_loss", "smooth_loss", "kl_loss"]
    t = Trainer({})
    assert t._aux_parts == () and t.teacher is None and t.teacher_kl_coeff == 0.0


def _round_trip_row(parts):
    from ssi.trainer import build_row, split_row
    kinds = ["dsu", "text"]
    counts = torch.tensor([5, 7, 12, 9])                            # per kind ..., total, valid labels
    aux = {name: torch.tensor(0.25 * (i + 1)) for i, name in enumerate(parts)}
    row = build_row(counts, torch.tensor(3.5), aux, torch.tensor(1.0), torch.tensor(2.0), parts)
    assert row.dtype == torch.float64 and row.numel() == len(kinds) + 5 + len(parts)
    got_counts, n_valid, loss, got_aux, bad_labels, bad_positions = split_row(row.tolist(), kinds, parts)
    assert got_counts == {"dsu": 5, "text": 7, "total": 12} and n_valid == 9 and loss == 3.5 and (bad_labels, bad_positions) == (1, 2)
    assert got_aux == {name: 0.25 * (i + 1) for i, name in enumerate(parts)} and list(got_aux) == list(parts)


def _round_trip_window(parts):
    from ssi.trainer import pack_window_scalars, unpack_window_scalars
    type_counts = {"text": 7, "dsu": 5}
    aux = {name: 1.5 * (i + 1) for i, name in enumerate(parts)}
    packed = pack_window_scalars(12, 3.5, 2, type_counts, aux, parts)
    assert len(packed) == 3 + len(type_counts) + len(parts)
    doubled = [2 * v for v in packed]                                # two ranks with the same window, summed
    n_tokens, loss, n_bad, counts, got_aux = unpack_window_scalars(doubled, sorted(type_counts), parts)
    assert (n_tokens, loss, n_bad, counts) == (24, 7.0, 4, {"dsu": 10, "text": 14})
    assert got_aux == {name: 3.0 * (i + 1) for i, name in enumerate(parts)}


def test_rows_and_window_scalars_round_trip_with_the_kl_part():
    from ssi.trainer import AUX_PARTS, TEACHER_PARTS
    for parts in (("kl_loss",), tuple(name for name, _ in AUX_PARTS + TEACHER_PARTS)):
        _round_trip_row(parts)
        _round_trip_window(parts)
