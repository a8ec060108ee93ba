"""The fp32 GEMM on the fp32-input matrix instruction (``csrc/gemm_f32_mfma.hip``): exact on integers against float64, and BIT-EQUAL to
the generic kernel on random data — both are one k-ordered fmaf chain per output element, started at 0 — through ``ssi_gemm`` and every
caller that falls through to it, up to a whole fp32 model step.

"Forced" = ``ops.set_impl(_lib.IMPL_MFMA)``: an fp32 call outside the support rule then raises, so a forced call that returns ran the
new kernel.  Support rule: N a multiple of 128 (M, K arbitrary)."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = [0, 1, 2]   # NT, NN, TN


@pytest.fixture(scope="module")
def ops():
    from ssi import ops as o
    return o


class _impl:
    def __init__(self, ops, impl):
        self.ops, self.impl = ops, impl

    def __enter__(self):
        self.prev = self.ops.set_impl(self.impl)

    def __exit__(self, *exc):
        self.ops.set_impl(self.prev)


def _shapes(layout, M, N, K):
    return ((M, K) if layout in (0, 1) else (K, M)), ((N, K) if layout == 0 else (K, N))


def _ref64(layout, a, b):
    a, b = a.double(), b.double()
    if layout == 0:
        return a @ b.T
    return a @ b if layout == 1 else a.T @ b


def _randn_dev(shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV)


# ---- 1. exact integers against float64 on the CPU --------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,N,K", [
    (128, 128, 64),                                    # one tile
    (1024, 8192, 96),                                  # 512 tiles: more than the chip runs at once
    (1, 256, 64), (70, 256, 64), (1000, 256, 64),      # M tails (TN with M % 4 != 0 takes the element-load form)
    (256, 128, 1), (256, 128, 33), (256, 128, 1000),   # K tails
    (1, 128, 1),                                       # the smallest supported shape
])
def test_integers_are_exact(ops, layout, M, N, K):
    """Operands in {-3 .. 3}, asymmetric: every product is <= 9 and every partial sum <= 9 K < 2^24, so every fp32 sum is exact."""
    from ssi import _lib
    g = torch.Generator().manual_seed(100 + layout)
    sa, sb = _shapes(layout, M, N, K)
    a = torch.randint(-3, 4, sa, generator=g).float()
    b = torch.randint(-3, 4, sb, generator=g).float()
    c = torch.full((M, N), float("nan"), device=DEV)
    with _impl(ops, _lib.IMPL_MFMA):
        ops.gemm(layout, a.to(DEV), b.to(DEV), c)
    assert torch.equal(c.cpu().double(), _ref64(layout, a, b))


# ---- 2. bit-equality with the generic kernel --------------------------------------------------------------------------------------------
def _modes(M, N, seed):
    r = _randn_dev((M, N), seed + 1)
    c0 = _randn_dev((M, N), seed + 2)
    four = torch.tensor([4.0], device=DEV)
    return [("plain", {}, None), ("alpha", dict(alpha=0.5, alpha_dev=four), None), ("accumulate", dict(accumulate=True), c0),
            ("residual", dict(residual=r), None), ("all", dict(residual=r, alpha=0.5, alpha_dev=four, accumulate=True), c0)]


def _both(ops, layout, a, b, M, N, kw, c0):
    from ssi import _lib
    outs = []
    for impl in (_lib.IMPL_MFMA, _lib.IMPL_GENERIC):
        c = c0.clone() if c0 is not None else torch.full((M, N), float("nan"), device=DEV)
        with _impl(ops, impl):
            ops.gemm(layout, a, b, c, **kw)
        outs.append(c)
    return outs


def _step_shapes(T):
    D, QKV, I2, I, V = 2048, 3072, 16384, 8192, 133376
    nt = [(0, T, n, k) for n, k in ((QKV, D), (D, D), (I2, D), (D, I), (V, D))]          # y = x W^T
    nn = [(1, T, n, k) for n, k in ((D, QKV), (D, D), (D, I2), (I, D), (D, V))]          # dx = dy W
    tn = [(2, m, n, T) for m, n in ((QKV, D), (D, D), (I2, D), (D, I), (V, D))]          # dW = dy^T x
    return nt + nn + tn


@pytest.mark.parametrize("layout,M,N,K", _step_shapes(1024) + _step_shapes(4096) + [
    (0, 11520, 3072, 2048), (2, 3072, 2048, 11520),    # the ragged headline batch: T is no multiple of the tile
    (2, 2048, 2048, 16384),                            # the longest chain of the step
    (0, 70, 256, 33), (1, 333, 128, 77), (2, 70, 384, 1001), (0, 200, 256, 96),   # tails, unaligned rows
])
def test_bits_equal_the_generic_kernel(ops, layout, M, N, K):
    sa, sb = _shapes(layout, M, N, K)
    a, b = _randn_dev(sa, 7), _randn_dev(sb, 8)
    modes = _modes(M, N, 9)
    if M * N > 1 << 28:   # the head at T = 4096 (2.2 GB per matrix): plain and everything at once
        modes = [modes[0], modes[4]]
    for name, kw, c0 in modes:
        new, old = _both(ops, layout, a, b, M, N, kw, c0)
        assert torch.equal(new, old), f"{name}: {int((new != old).sum())} of {new.numel()} elements differ, max |d| {float((new - old).abs().max())}"
        assert bool(torch.isfinite(new).all())


@pytest.mark.parametrize("layout", LAYOUTS)
def test_subnormals_are_kept_like_the_generic_kernel(ops, layout):
    """Subnormal operands (|a| ~ 1e-40) and subnormal products / sums (1e-20 x 1e-20): neither kernel flushes them."""
    M, N, K = 200, 256, 160
    sa, sb = _shapes(layout, M, N, K)
    g = torch.Generator().manual_seed(31)
    for sc_a, sc_b in ((1e-40, 1e2), (1e-20, 1e-20)):
        a = (torch.randn(sa, generator=g).double() * sc_a).float().to(DEV)
        b = (torch.randn(sb, generator=g).double() * sc_b).float().to(DEV)
        new, old = _both(ops, layout, a, b, M, N, {}, None)
        assert torch.equal(new, old)
        assert float((new != 0).float().mean()) > 0.9, "the subnormal results were flushed to zero"
        assert float(new.abs().max()) < 1.2e-38 * 100


@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_zero_row_and_negative_zero_in_c(ops, layout):
    M, N, K = 130, 128, 100
    sa, sb = _shapes(layout, M, N, K)
    a, b = _randn_dev(sa, 41), _randn_dev(sb, 42)
    if layout == 2:
        a[:, 5] = 0.0
    else:
        a[5, :] = 0.0
    c0 = torch.full((M, N), -0.0, device=DEV)
    for kw in ({}, dict(accumulate=True)):
        new, old = _both(ops, layout, a, b, M, N, kw, c0)
        assert torch.equal(new, old) and bool((new[5] == 0).all()) and bool((new[4] != 0).any())


# ---- 3. against float64 at the tolerance of test_gemm_generic ---------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("M,N,K", [(70, 256, 33), (256, 256, 512), (1000, 512, 512)])
def test_against_float64(ops, layout, M, N, K):
    from ssi import _lib
    g = torch.Generator().manual_seed(18)
    sa, sb = _shapes(layout, M, N, K)
    a, b = torch.randn(sa, generator=g), torch.randn(sb, generator=g)
    c = torch.full((M, N), float("nan"), device=DEV)
    with _impl(ops, _lib.IMPL_MFMA):
        ops.gemm(layout, a.to(DEV), b.to(DEV), c)
    ref = _ref64(layout, a, b)
    print(f"max |err| {float((c.cpu().double() - ref).abs().max()):.3e}")
    torch.testing.assert_close(c.cpu().double(), ref, rtol=1e-5, atol=1e-4)
    r, c0 = torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
    c1 = c0.to(DEV)
    with _impl(ops, _lib.IMPL_MFMA):
        ops.gemm(layout, a.to(DEV), b.to(DEV), c1, residual=r.to(DEV), alpha=0.5, alpha_dev=torch.tensor([4.0], device=DEV), accumulate=True)
    torch.testing.assert_close(c1.cpu().double(), c0.double() + 2.0 * ref + r.double(), rtol=1e-5, atol=1e-4)


# ---- 4. dispatch ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
def test_dispatch(ops, layout):
    from ssi import _lib
    out = {}
    for tag, (M, N, K) in (("supported", (200, 256, 96)), ("unsupported", (200, 130, 96))):
        sa, sb = _shapes(layout, M, N, K)
        a, b = _randn_dev(sa, 51), _randn_dev(sb, 52)
        for impl in (_lib.IMPL_AUTO, _lib.IMPL_GENERIC, _lib.IMPL_MFMA, _lib.IMPL_MFMA_WG8):
            c = torch.full((M, N), float("nan"), device=DEV)
            with _impl(ops, impl):
                if tag == "unsupported" and impl in (_lib.IMPL_MFMA, _lib.IMPL_MFMA_WG8):
                    with pytest.raises(RuntimeError, match="unsupported"):
                        ops.gemm(layout, a, b, c)
                    continue
                ops.gemm(layout, a, b, c)
            out[tag, impl] = c
    assert torch.equal(out["supported", _lib.IMPL_AUTO], out["supported", _lib.IMPL_MFMA])
    assert torch.equal(out["supported", _lib.IMPL_MFMA_WG8], out["supported", _lib.IMPL_MFMA])
    assert torch.equal(out["supported", _lib.IMPL_GENERIC], out["supported", _lib.IMPL_MFMA])
    assert torch.equal(out["unsupported", _lib.IMPL_AUTO], out["unsupported", _lib.IMPL_GENERIC])


def test_bf16_calls_are_what_they_were_before_any_fp32_call():
    """In a process of its own (this one has long made fp32 calls): tests/workers/gemm_f32_dispatch_worker.py."""
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "workers", "gemm_f32_dispatch_worker.py")], capture_output=True,
                          text=True, timeout=300)
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]


# ---- 5. the callers that fall through to ssi_gemm in fp32 -------------------------------------------------------------------------------
def _three_ways(ops, run):
    """run() -> tuple of output tensors; AUTO and GENERIC bit-equal, forced does not raise and agrees too."""
    from ssi import _lib
    res = {}
    for impl in (_lib.IMPL_AUTO, _lib.IMPL_GENERIC, _lib.IMPL_MFMA):
        with _impl(ops, impl):
            res[impl] = run()
    for x, y, z in zip(res[_lib.IMPL_AUTO], res[_lib.IMPL_GENERIC], res[_lib.IMPL_MFMA]):
        assert torch.equal(x, y) and torch.equal(z, y) and bool(torch.isfinite(x).all())


def test_gemm_batched_inherits_it(ops):
    a, b = _randn_dev((4, 300, 256), 61), _randn_dev((4, 300, 384), 62)   # TN: c[i] = a[i]^T b[i]
    c0 = _randn_dev((4, 256, 384), 63)

    def run():
        c, c1 = torch.full((4, 256, 384), float("nan"), device=DEV), c0.clone()
        ops.gemm_batched(2, a, b, c)
        ops.gemm_batched(2, a, b, c1, alpha=0.5, accumulate=True)
        return c, c1
    _three_ways(ops, run)


def test_gemm_splitk_inherits_it(ops):
    a, b = _randn_dev((1024, 256), 64), _randn_dev((1024, 256), 65)
    ws = torch.empty(4 * 256 * 256, device=DEV)

    def run():
        c = torch.full((256, 256), float("nan"), device=DEV)
        ops.gemm_splitk(2, a, b, c, 4, ws)   # fp32 forwards to ssi_gemm: no slices, no other summation order
        return (c,)
    _three_ways(ops, run)


def test_gemm_rope_inherits_it(ops):
    S, H, KV, hd, D = 96, 4, 2, 64, 256
    x, w = _randn_dev((2 * S, D), 66), _randn_dev(((H + 2 * KV) * hd, D), 67)
    from ssi.model import llama3_rope_table
    table = llama3_rope_table(hd, 128).to(DEV)   # [len, hd / 2, (cos, sin)]

    def run():
        c = torch.full((2 * S, (H + 2 * KV) * hd), float("nan"), device=DEV)
        ops.gemm_rope(x, w, c, S, H + KV, hd, table)
        return (c,)
    _three_ways(ops, run)


def test_gemm_swiglu_inherits_it(ops):
    M, I, D = 200, 512, 256
    x, w13 = _randn_dev((M, D), 68), _randn_dev((2 * I, D), 69) * 0.1
    dy, w2 = _randn_dev((M, D), 70), _randn_dev((D, I), 71) * 0.1

    def run():
        gu, act = torch.full((M, 2 * I), float("nan"), device=DEV), torch.full((M, I), float("nan"), device=DEV)
        ops.gemm_swiglu_fwd(x, w13, gu, act)
        dgu, dgu2 = torch.full_like(gu, float("nan")), torch.full_like(gu, float("nan"))
        ops.gemm_swiglu_bwd(1, dy, w2, gu, dgu, torch.empty(M, I, device=DEV))                    # NN: w2 as stored, [D, I]
        ops.gemm_swiglu_bwd(0, dy, w2.t().contiguous(), gu, dgu2, torch.empty(M, I, device=DEV))  # NT: the transposed copy
        return gu, act, dgu, dgu2
    _three_ways(ops, run)


# ---- 6. the model ---------------------------------------------------------------------------------------------------------------------
PARAMS = dict(vocab_size=700, num_layers=2, num_heads=4, num_kv_heads=2, embed_dim=256, max_seq_len=512, intermediate_dim=512)


def _model_step(ops, impl, log=None):
    from oracle import hf_crosscheck as hx
    from ssi.loss import CEWithChunkedOutputLoss, compute_loss
    from ssi.model import HipLlamaDecoder
    from ssi.optimizer import HipAdamW
    real = {n: getattr(ops, n) for n in ("gemm", "gemm_splitk", "gemm_batched", "gemm_rope", "gemm_swiglu_fwd", "gemm_swiglu_bwd")}

    def mnk(layout, a, c):
        return (layout, c.shape[-2], c.shape[-1], a.shape[-1] if layout in (0, 1) else a.shape[-2])

    def wrap(name):
        def f(*args, **kw):
            if name in ("gemm", "gemm_splitk", "gemm_batched"):
                log.add(mnk(args[0], args[1], args[3]))
            elif name == "gemm_rope":
                log.add(mnk(0, args[0], args[2]))
            elif name == "gemm_swiglu_fwd":
                log.add(mnk(0, args[0], args[2]))
            else:   # gemm_swiglu_bwd(layout, dy, w2, gu, dgu, ws): [M, K] x W2 -> [M, I]
                log.add((args[0], args[1].shape[0], args[3].shape[1] // 2, args[1].shape[1]))
            return real[name](*args, **kw)
        return f

    with _impl(ops, impl):
        try:
            if log is not None:
                for n in real:
                    setattr(ops, n, wrap(n))
            model = HipLlamaDecoder(**PARAMS, dtype=torch.float32, device=DEV)
            model.load_state_dict(hx.seeded_state_dict(PARAMS, 12))
            model.set_num_output_chunks(8)
            model.train()
            batch = {k: v.to(DEV) for k, v in hx.seeded_batch(PARAMS["vocab_size"], 2, 96, 12).items()}
            with torch.no_grad():
                logits = torch.cat(model(tokens=batch["tokens"]), dim=1).clone()
            loss = compute_loss(batch, model, CEWithChunkedOutputLoss())
            loss.backward()
            grads = {k: p.grad.clone() for k, p in model.named_parameters()}
            opt = HipAdamW(model.parameters(), model=model, lr=1e-2)
            opt.step()
            params = {k: p.detach().clone() for k, p in model.named_parameters()}
            torch.cuda.synchronize()
        finally:
            for n, f in real.items():
                setattr(ops, n, f)
    return loss.detach().clone(), logits, grads, params


def test_fp32_model_step_is_bit_equal_and_runs_on_the_new_kernel(ops):
    from ssi import _lib
    log = set()
    auto = _model_step(ops, _lib.IMPL_AUTO, log)
    generic = _model_step(ops, _lib.IMPL_GENERIC)
    assert torch.equal(auto[0], generic[0]) and torch.equal(auto[1], generic[1]) and bool(torch.isfinite(auto[0]))
    for part in (2, 3):
        assert auto[part].keys() == generic[part].keys()
        for k in auto[part]:
            assert torch.equal(auto[part][k], generic[part][k]), k
    # every GEMM the model issued is inside the support rule: the forced call returns, and returns the generic kernel's bits
    assert len(log) >= 8 and {s[0] for s in log} == {0, 1, 2}, sorted(log)
    for layout, M, N, K in sorted(log):
        sa, sb = _shapes(layout, M, N, K)
        a, b = _randn_dev(sa, 81), _randn_dev(sb, 82)
        new, old = _both(ops, layout, a, b, M, N, {}, None)
        assert torch.equal(new, old), (layout, M, N, K)
