"""fp32 GEMMs of one training step: the generic kernel (IMPL_GENERIC, vector ALU) against the fp32 MFMA kernel (IMPL_AUTO) in ONE process.

The shape list comes from the model: every GEMM that one fp32 forward + backward of a 1-layer model at T = batch x seq tokens issues is logged
as (layout, M, N, K, accumulate, residual) — ``ops.gemm`` / ``gemm_batched`` / ``gemm_splitk`` directly, the fused-epilogue entry points
(``gemm_rope``, ``gemm_swiglu_fwd`` / ``_bwd``) as the plain GEMM they fall through to in fp32 — and the distinct ones are kept; 4096^3 is
added so that the rate can be read against published figures.  Every shape is warmed up under both settings, then timed with HIP events in
windows of enough launches to last about ``--window`` seconds, the two settings ALTERNATING window by window; the median of ``--windows``
windows is reported with the spread (min .. max) beside it.

    python tools/gemm_f32_ab.py [--out profiles/fp32_gemm_ab.json]"""
import argparse
import copy
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "speech-integration_amd"))

import torch  # noqa: E402

PEAK_TF = 157.3   # fp32-input MFMA peak of the MI355X
LAYOUT = {0: "NT", 1: "NN", 2: "TN"}


def step_shapes(batch: int, seq: int, n_dsus: int = 5000) -> list[tuple]:
    from ssi import ops
    from ssi.data import loss_inputs, synthetic_batch
    from ssi.llama_configs import configllama3_2_1b
    from ssi.loss import CEWithChunkedOutputLoss, compute_loss
    from ssi.model import HipLlamaDecoder
    lcfg = copy.deepcopy(configllama3_2_1b)
    lcfg.n_dsus, lcfg.modality_tokens, lcfg.num_layers = n_dsus, True, 1
    model = HipLlamaDecoder(**lcfg.parameters, dtype=torch.float32, device="cuda", rope_cache_len=max(seq, 2048))
    with torch.no_grad():
        model._flat.normal_(0.0, 0.02)
    model.train()
    loss_fn = CEWithChunkedOutputLoss()
    model.set_num_output_chunks(loss_fn.num_output_chunks)
    seen: dict[tuple, int] = {}
    real = {n: getattr(ops, n) for n in ("gemm", "gemm_splitk", "gemm_batched", "gemm_rope", "gemm_swiglu_fwd", "gemm_swiglu_bwd")}

    def note(layout, a, c, accumulate=False, residual=None, count=1):
        key = (layout, c.shape[-2], c.shape[-1], a.shape[-1] if layout in (0, 1) else a.shape[-2], bool(accumulate), residual is not None)
        seen[key] = seen.get(key, 0) + count

    def wrap(name):
        def f(*args, **kw):
            if name in ("gemm", "gemm_batched"):
                note(args[0], args[1], args[3], kw.get("accumulate"), kw.get("residual"), args[3].shape[0] if name == "gemm_batched" else 1)
            elif name == "gemm_splitk" and args[4] > 1:   # (splits <= 1 goes through ops.gemm and is logged there)
                note(args[0], args[1], args[3], kw.get("accumulate"), kw.get("residual"))
            elif name in ("gemm_rope", "gemm_swiglu_fwd"):
                note(0, args[0], args[2])
            elif name == "gemm_swiglu_bwd":
                note(args[0], args[1], args[3][:, : args[3].shape[1] // 2])
            return real[name](*args, **kw)
        return f

    try:
        for n in real:
            setattr(ops, n, wrap(n))
        b = {k: (v.to("cuda") if torch.is_tensor(v) else v) for k, v in synthetic_batch(batch, seq, n_dsus, rank=0, index=0, fixed_len=True).items()}
        compute_loss(loss_inputs(b), model, loss_fn).backward()
        torch.cuda.synchronize()
    finally:
        for n, f in real.items():
            setattr(ops, n, f)
    del model
    torch.cuda.empty_cache()
    return [k + (v,) for k, v in sorted(seen.items())]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=2048)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.15, help="seconds per timed window (at least one launch)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp32_gemm_ab.json"))
    args = ap.parse_args()
    from ssi import _lib, ops
    shapes = [s + ("step",) for s in step_shapes(args.batch, args.seq)] + [(0, 4096, 4096, 4096, False, False, 0, "4096^3")]
    settings = (("generic", _lib.IMPL_GENERIC), ("mfma", _lib.IMPL_AUTO))
    rows = []
    for layout, M, N, K, accumulate, residual, calls, origin in shapes:
        a = torch.randn((M, K) if layout < 2 else (K, M), device="cuda")
        b = torch.randn((N, K) if layout == 0 else (K, N), device="cuda")
        c = torch.zeros(M, N, device="cuda")
        r = torch.randn(M, N, device="cuda") if residual else None
        run = lambda: ops.gemm(layout, a, b, c, accumulate=accumulate, residual=r)   # noqa: E731

        def window(impl, n):
            prev = ops.set_impl(impl)
            try:
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(n):
                    run()
                e.record()
                torch.cuda.synchronize()
            finally:
                ops.set_impl(prev)
            return s.elapsed_time(e) * 1e-3 / n

        n_launch = {}
        for name, impl in settings:   # warm-up under both settings; the second launch sizes the window
            window(impl, 1)
            n_launch[name] = max(1, min(2000, math.ceil(args.window / window(impl, 1))))
        times = {name: [] for name, _ in settings}
        for _ in range(args.windows):
            for name, impl in settings:
                times[name].append(window(impl, n_launch[name]))
        flop = 2.0 * M * N * K
        row = {"origin": origin, "layout": LAYOUT[layout], "M": M, "N": N, "K": K, "accumulate": accumulate, "residual": residual, "calls_per_layer_step": calls}
        for name, _ in settings:
            med = statistics.median(times[name])
            row[name] = {"us": round(med * 1e6, 1), "tf": round(flop / med / 1e12, 2), "tf_min": round(flop / max(times[name]) / 1e12, 2),
                         "tf_max": round(flop / min(times[name]) / 1e12, 2), "launches_per_window": n_launch[name], "windows": args.windows}
        row["ratio"] = round(row["mfma"]["tf"] / row["generic"]["tf"], 2)
        row["mfma_fraction_of_peak"] = round(row["mfma"]["tf"] / PEAK_TF, 3)
        rows.append(row)
        print(f"{origin:7s} {LAYOUT[layout]} {M:6d} x {N:6d} x {K:6d} acc={int(accumulate)} res={int(residual)}  generic {row['generic']['tf']:6.2f} TF "
              f"[{row['generic']['tf_min']:.2f} .. {row['generic']['tf_max']:.2f}]  mfma {row['mfma']['tf']:7.2f} TF [{row['mfma']['tf_min']:.2f} .. "
              f"{row['mfma']['tf_max']:.2f}] = {row['mfma_fraction_of_peak']:.0%} of {PEAK_TF}  x{row['ratio']:.2f}", flush=True)
        del a, b, c, r
    result = {"device": torch.cuda.get_device_name(0), "peak_tf": PEAK_TF, "tokens": args.batch * args.seq, "window_s": args.window, "shapes": rows,
              "mfma_faster_at_every_step_shape": all(r["ratio"] > 1.0 for r in rows if r["origin"] == "step")}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k != "shapes"}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
