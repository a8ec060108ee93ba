"""GPU: ``optimizer.stochastic_rounding`` through ``Trainer.train()`` (bf16, the MFMA_SMALL geometry of tests/test_trainer_gpu.py at seq 128).
The random bits are a pure function of (seed, step, element index in the flat buffer, tensor), so everything that was bit-reproducible with
round-to-nearest stays so: two fresh runs, a resume, the AdamW that runs under the backward, the three slices of the data-parallel step.
Flag and seed belong to the run's configuration, not to the saved state: either kind of state resumes into either kind of run."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

MFMA_SMALL = {"num_layers": 2, "num_heads": 4, "num_kv_heads": 2, "embed_dim": 256, "intermediate_dim": 512, "max_seq_len": 512,
              "_base_vocab_size_txt": 300, "_n_special_txt": 16}
SR = "optimizer.stochastic_rounding=true"


class _Remap:
    """The synthetic generator draws ids from the production vocabulary layout; fold them into the shrunken test vocabulary."""

    def __init__(self, loader, vocab):
        self.loader, self.dataset, self.vocab = loader, loader.dataset, vocab

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        for b in self.loader:
            tok = b["tokens"] % self.vocab
            yield {"tokens": tok, "labels": torch.where(b["labels"] == -100, b["labels"], tok)}


def _trainer(tmp, name, dtype="bf16", overrides=(), model=MFMA_SMALL, seq=128):
    from conftest import PKG
    from ssi.config import compose
    from ssi.constants import SEED
    from ssi.train_utils import resolve_n_dsus
    from ssi.trainer import Trainer, set_seed
    out = tmp / name
    cfg = compose(os.path.join(PKG, "conf"), "sft", [
        "data=sft/mls-speechtokenizer-rvq_0", f"dtype={dtype}", f"tokenizer.max_seq_len={seq}", "data.train.dataloader.batch_size=2",
        "data.dev.dataloader.batch_size=2", "data.train.dataset.n_samples=24", "data.dev.dataset.n_samples=6", "gradient_accumulation_steps=2",
        "eval_steps=1000", "save_steps=1000", "lr_scheduler.num_warmup_steps=100", "optimizer.lr=2e-2", f"output_dir={out}",
        f"checkpointer.output_dir={out}/checkpoints", f"checkpointer.checkpoint_dir={out}/none", "checkpointer.allow_random_init=true", *overrides])
    cfg.model_overrides = dict(model)
    cfg.speech.n_dsus = 50
    cfg.data.n_dsus = 50
    resolve_n_dsus(cfg)
    set_seed(SEED)
    t = Trainer(cfg)
    t.setup()
    V = t._llama_config.vocab_size
    t.data_train, t.data_dev = _Remap(t.data_train, V), _Remap(t.data_dev, V)
    t._loss_log = []
    return t


def _finish(t):
    t.train()
    out = dict(losses=list(t._loss_log), w={k: v.detach().clone() for k, v in t.model.state_dict().items()}, steps=t.optimizer._step_count,
               m=t.optimizer._exp_avg.clone(), v=t.optimizer._exp_avg_sq.clone(), seed=t.optimizer._sr_seed)
    t.cleanup()
    return out


def _same(a, b):
    return (a["losses"] == b["losses"] and all(torch.equal(a["w"][k], b["w"][k]) for k in a["w"])
            and torch.equal(a["m"], b["m"]) and torch.equal(a["v"], b["v"]))


class _DeferredMlpBucket:
    """What ``HipAdamW.step`` sees of a data-parallel exchange with one bucket still in flight: the range it must update last."""

    def __init__(self, model):
        _, self.lo, self.hi = model._bucket_by_name["L0.mlp"]
        self.asked = self.finished = 0

    def deferred_range(self):
        self.asked += 1
        return self.lo, self.hi

    def finish_deferred(self):
        self.finished += 1

    def bucket_ready(self, *bucket):
        pass


@pytest.fixture(scope="module")
def six_steps(tmp_path_factory):
    """Six optimizer steps, once per configuration; shared by T1, T3 and T4."""
    from ssi.constants import SEED
    tmp = tmp_path_factory.mktemp("sr6")
    runs = {}
    for name, extra in (("on", [SR]), ("again", [SR]), ("off", []), ("after_backward", [SR, "adamw_under_backward=false"]),
                        ("other_seed", [SR, "optimizer.stochastic_rounding_seed=7"])):
        t = _trainer(tmp, name, overrides=["max_steps=6", *extra])
        armed, real = [], t.optimizer.overlap_with_backward
        t.optimizer.overlap_with_backward = lambda s, real=real, armed=armed: (armed.append(real(s)), armed[-1])[1]
        runs[name] = _finish(t)
        runs[name]["armed"] = sum(bool(a) for a in armed)
        del t
    t = _trainer(tmp, "deferred", overrides=["max_steps=6", SR])
    stub = _DeferredMlpBucket(t.model)
    assert 0 < stub.lo < stub.hi < t.model._flat.numel() and stub.lo % 8 == 0 and stub.hi % 8 == 0
    t.model.grad_sync = stub
    runs["deferred"] = _finish(t)
    runs["deferred"]["stub"] = stub
    assert runs["on"]["seed"] == SEED and runs["off"]["seed"] is None and runs["other_seed"]["seed"] == 7
    return runs


def test_two_fresh_runs_are_bit_identical_and_differ_from_nearest(six_steps):          # T1
    on, again, off = six_steps["on"], six_steps["again"], six_steps["off"]
    assert on["steps"] == again["steps"] == off["steps"] == 6 and len(set(on["losses"])) == 6
    assert _same(on, again)
    assert on["losses"] != off["losses"] and any(not torch.equal(on["w"][k], off["w"][k]) for k in on["w"])
    assert on["losses"][0] == off["losses"][0]                  # (the first loss is taken before any update)
    assert not _same(on, six_steps["other_seed"])               # the seed is the configuration's


def test_under_the_backward_or_after_it_the_same_bits(six_steps):                        # T3
    on, after = six_steps["on"], six_steps["after_backward"]
    assert on["armed"] == 6 and after["armed"] == 0
    assert _same(on, after)


def test_the_three_slices_of_the_data_parallel_step_are_the_plain_step(six_steps):       # T4
    deferred = six_steps["deferred"]
    assert deferred["stub"].asked == 6 and deferred["stub"].finished >= 6
    assert _same(six_steps["on"], deferred)


@pytest.fixture(scope="module")
def saved_at_four(tmp_path_factory):
    """Four steps and a save, with the key on and with it off."""
    tmp = tmp_path_factory.mktemp("sr4")
    out = {"tmp": tmp}
    for name, extra in (("on", [SR]), ("off", [])):
        t = _trainer(tmp, f"b1_{name}", overrides=["max_steps=4", "save_steps=4", "eval_steps=4", *extra])
        out[name] = _finish(t)
        ckpt = tmp / f"b1_{name}" / "checkpoints"
        assert (ckpt / "training_state.pt").exists() and (ckpt / "step_4" / "model.safetensors").exists()
        out[name]["ckpt"] = ckpt
        del t
    return out


def _resume(saved, kind, name, extra):
    ckpt = saved[kind]["ckpt"]
    t = _trainer(saved["tmp"], name, overrides=["max_steps=8", f"checkpointer.checkpoint_dir={ckpt}/step_4", "checkpointer.allow_random_init=false",
                                                f"checkpointer.training_state_checkpoint={ckpt}/training_state.pt", *extra])
    assert t.global_step == 4 and t.optimizer._step_count == 4 and float(t.optimizer._exp_avg.abs().max()) > 0
    return t


def test_resumed_run_is_the_uninterrupted_one(saved_at_four):                            # T2
    full = _finish(_trainer(saved_at_four["tmp"], "full", overrides=["max_steps=8", SR]))
    assert len(full["losses"]) == 8 and len(set(full["losses"])) == 8
    assert saved_at_four["on"]["losses"] == full["losses"][:4], "pre-resume losses differ"
    t = _resume(saved_at_four, "on", "b2", [SR])
    assert t.optimizer._sr_seed is not None
    assert torch.equal(t.optimizer._exp_avg, saved_at_four["on"]["m"]) and torch.equal(t.optimizer._exp_avg_sq, saved_at_four["on"]["v"])
    resumed = _finish(t)
    print("full   ", full["losses"], "\nresumed", resumed["losses"])
    assert resumed["losses"] == full["losses"][4:], "losses after the resume differ from the uninterrupted run"
    assert resumed["steps"] == 8
    assert all(torch.equal(resumed["w"][k], full["w"][k]) for k in full["w"])
    assert torch.equal(resumed["m"], full["m"]) and torch.equal(resumed["v"], full["v"])


def test_a_state_saved_either_way_resumes_either_way(saved_at_four):                      # T6
    """The saved ``param_groups`` carry neither key, and a loaded state does not decide the rounding: the run's configuration does."""
    state = torch.load(saved_at_four["on"]["ckpt"] / "training_state.pt", map_location="cpu", weights_only=False)
    from ssi.constants import OPTIMIZER_KEY
    groups = state[OPTIMIZER_KEY]["param_groups"]
    assert all("stochastic_rounding" not in g and "stochastic_rounding_seed" not in g for g in groups)
    t = _resume(saved_at_four, "off", "off_then_on", [SR])
    assert t.optimizer._sr_seed is not None
    on = _finish(t)
    t = _resume(saved_at_four, "off", "off_then_off", [])
    assert t.optimizer._sr_seed is None
    off = _finish(t)
    t = _resume(saved_at_four, "on", "on_then_off", [])
    assert t.optimizer._sr_seed is None
    back = _finish(t)
    for run in (on, off, back):
        assert run["steps"] == 8 and len(run["losses"]) == 4 and all(x == x and abs(x) < 1e3 for x in run["losses"])
    assert on["losses"][0] == off["losses"][0] and on["losses"] != off["losses"]     # same state in, another rounding from the first step on
    assert any(not torch.equal(on["w"][k], off["w"][k]) for k in on["w"])


def test_the_key_is_refused_where_it_cannot_be_honoured(tmp_path):                        # T5
    from ssi.optimizer import HipAdamW, setup_optimizer
    small = {"num_layers": 2, "num_heads": 4, "num_kv_heads": 2, "embed_dim": 64, "intermediate_dim": 128, "max_seq_len": 256,
             "_base_vocab_size_txt": 300, "_n_special_txt": 16}
    with pytest.raises(ValueError, match="stochastic_rounding"):
        _trainer(tmp_path, "fp32", dtype="fp32", model=small, seq=96, overrides=["max_steps=1", SR])
    t = _trainer(tmp_path, "fp32_off", dtype="fp32", model=small, seq=96, overrides=["max_steps=1"])      # the key off: as before
    assert t.optimizer._sr_seed is None
    with pytest.raises(ValueError, match="stochastic_rounding"):
        HipAdamW(t.model.parameters(), model=t.model, stochastic_rounding=True)
    foreign = torch.nn.Linear(8, 8)
    t.cfg.optimizer.stochastic_rounding = True
    with pytest.raises(ValueError, match="stochastic_rounding"):
        setup_optimizer(t.cfg, foreign)
    t.cfg.optimizer.stochastic_rounding = False
    assert type(setup_optimizer(t.cfg, foreign)) is torch.optim.AdamW                                      # both keys stripped
    t.cleanup()
