"""CPU, no library: the trainer's read-back row and its data-parallel scalar vector are described by two helpers each (``build_row`` /
``split_row``, ``pack_window_scalars`` / ``unpack_window_scalars`` of ``ssi/trainer.py``).  With two token kinds and every combination of
z-loss on / off x label smoothing on / off: every field, given a value of its own, comes back under its own name, and the widths are the
ones the layout comments state."""
import itertools

import pytest
import torch

KINDS = ["text", "dsu"]
COMBOS = [tuple(name for name, on in (("z_loss", z_on), ("smooth_loss", smooth_on)) if on)
          for z_on, smooth_on in itertools.product((False, True), repeat=2)]


def test_the_part_names_and_their_order_are_fixed():
    from ssi.trainer import AUX_PARTS, Trainer
    assert AUX_PARTS == (("z_loss", "z_loss_coeff"), ("smooth_loss", "label_smoothing"))
    t = Trainer({})
    assert t._aux_parts == () and t._aux_running == {}
    assert sorted(COMBOS) == sorted([(), ("z_loss",), ("smooth_loss",), ("z_loss", "smooth_loss")])


@pytest.mark.parametrize("parts", COMBOS, ids=lambda p: "+".join(p) or "plain")
def test_a_row_built_from_named_pieces_splits_back_into_them(parts):
    from ssi.trainer import build_row, split_row
    counts = torch.tensor([11, 13, 29, 17])                                      # per kind ..., total (non-pad), valid labels
    aux = {"smooth_loss": torch.tensor(0.375), "z_loss": torch.tensor(2.5)}       # (given in the other order: names decide, not positions)
    row = build_row(counts, torch.tensor(41.25, requires_grad=True), {k: aux[k] for k in aux if k in parts}, torch.tensor(3), torch.tensor(5.0), parts)
    assert row.dtype == torch.float64 and row.shape == (len(KINDS) + 5 + len(parts),) and not row.requires_grad
    got_counts, n_valid, loss, got_aux, bad_labels, bad_positions = split_row(row.tolist(), KINDS, parts)
    assert got_counts == {"text": 11, "dsu": 13, "total": 29} and all(type(v) is int for v in got_counts.values())
    assert (n_valid, loss, bad_labels, bad_positions) == (17, 41.25, 3, 5) and type(n_valid) is int and type(bad_labels) is int
    assert got_aux == {k: float(aux[k]) for k in parts} and list(got_aux) == list(parts)
    with pytest.raises(AssertionError):                                           # a row of another width is not read at all
        split_row(row.tolist() + [0.0], KINDS, parts)
    with pytest.raises(AssertionError):
        split_row(row.tolist(), KINDS + ["other"], parts)


@pytest.mark.parametrize("parts", COMBOS, ids=lambda p: "+".join(p) or "plain")
def test_the_all_reduce_vector_unpacks_into_what_was_packed(parts):
    from ssi.trainer import pack_window_scalars, unpack_window_scalars
    type_counts = {"total": 29, "text": 11, "dsu": 13}                            # the window's counts carry "total" too; packed in sorted order
    aux = {"z_loss": 2.5, "smooth_loss": 0.375}
    values = pack_window_scalars(17, 41.25, 7, type_counts, {k: aux[k] for k in parts}, parts)
    assert len(values) == 3 + len(type_counts) + len(parts) and all(type(v) is float for v in values)
    summed = [2.0 * v for v in values]                                            # two ranks that saw the same window
    n_tokens, loss, n_bad, got_counts, got_aux = unpack_window_scalars(summed, sorted(type_counts), parts)
    assert (n_tokens, loss, n_bad) == (34, 82.5, 14) and type(n_tokens) is int and type(n_bad) is int
    assert got_counts == {k: 2 * v for k, v in type_counts.items()}
    assert got_aux == {k: 2.0 * aux[k] for k in parts} and list(got_aux) == list(parts)
    with pytest.raises(AssertionError):
        unpack_window_scalars(summed + [0.0], sorted(type_counts), parts)
