"""Cross-entropy kernel alone at the step's shape: T = 16384 rows, V = 133258 (ld 133376), bf16, gradient in place.
``--z COEFF``: the z-loss form (``ops.ce_fwd_z``, ``ssi_ce_fwd_z``) with that coefficient instead of ``ops.ce_fwd``.
``--smooth E``: the label-smoothing form (``ops.ce_fwd_smooth``, ``ssi_ce_fwd_smooth``) with that smoothing, and ``--z`` (default 0) as its z.
``--metrics``: the label-rank form (``ops.ce_fwd_metrics``, ``ssi_ce_fwd_metrics``; forward only: one pass over the logits).
``--kl BETA``: the KL form against a second buffer of teacher logits (``ops.ce_fwd_kl``, ``ssi_ce_fwd_kl``) TOGETHER WITH the forward-only
``ops.ce_fwd`` on the teacher buffer that gives its lse — the two launches a training step with a teacher adds in place of ``ops.ce_fwd``; each
of the two is also timed on its own."""
import argparse, sys, torch
sys.path.insert(0, 'speech-integration_amd')
from ssi import ops
ap = argparse.ArgumentParser()
ap.add_argument("--z", type=float, default=None, metavar="COEFF", help="time ce_fwd_z with this coefficient (default: ce_fwd)")
ap.add_argument("--smooth", type=float, default=None, metavar="E", help="time ce_fwd_smooth with this smoothing (and --z, default 0)")
ap.add_argument("--metrics", action="store_true", help="time ce_fwd_metrics")
ap.add_argument("--kl", type=float, default=None, metavar="BETA", help="time the teacher-lse launch + ce_fwd_kl with this coefficient")
ap.add_argument("--reps", type=int, default=10)
args = ap.parse_args()
T, V, LD = 16384, 133258, 133376
logits = (torch.randn(T, LD, device='cuda') * 2).bfloat16()
labels = torch.randint(0, V, (T,), device='cuda')
labels[::7] = -100
row_loss = torch.empty(T, device='cuda'); row_lse = torch.empty(T, device='cuda'); row_z = torch.empty(T, device='cuda')
row_u = torch.empty(T, device='cuda')
row_nll = torch.empty(T, device='cuda'); row_rank = torch.empty(T, device='cuda', dtype=torch.int32)
work = logits.clone()
if args.kl is not None:
    teacher = (logits.float() + 0.5 * torch.randn(T, LD, device='cuda')).bfloat16()
    teacher_lse = torch.empty(T, device='cuda'); teacher_loss = torch.empty(T, device='cuda'); row_kl = torch.empty(T, device='cuda')
def run_teacher_lse():
    ops.ce_fwd(teacher, labels, V, -100, teacher_loss, teacher_lse, write_grad=False)
def run_kl():
    ops.ce_fwd_kl(work, teacher, teacher_lse, labels, V, -100, args.kl, row_loss, row_lse, row_kl, write_grad=True)
def run():
    if args.kl is not None:
        run_teacher_lse(); run_kl()
    elif args.metrics:
        ops.ce_fwd_metrics(work, labels, V, -100, row_loss, row_lse, row_nll, row_rank)
    elif args.smooth is not None:
        ops.ce_fwd_smooth(work, labels, V, -100, args.smooth, args.z or 0.0, row_loss, row_lse, row_u, row_z, write_grad=True)
    elif args.z is None:
        ops.ce_fwd(work, labels, V, -100, row_loss, row_lse, write_grad=True)
    else:
        ops.ce_fwd_z(work, labels, V, -100, args.z, row_loss, row_lse, row_z, write_grad=True)
for _ in range(3):
    work.copy_(logits); run()
torch.cuda.synchronize()
s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
ms = []
for _ in range(args.reps):
    work.copy_(logits)
    s.record(); run(); e.record(); torch.cuda.synchronize()
    ms.append(s.elapsed_time(e))
mean = sum(ms) / len(ms)
if args.kl is not None:
    for what, fn in (("teacher lse (ce_fwd, write_grad=False)", run_teacher_lse), (f"ce_fwd_kl({args.kl:g})", run_kl)):
        part = []
        for _ in range(args.reps):
            work.copy_(logits)
            s.record(); fn(); e.record(); torch.cuda.synchronize()
            part.append(s.elapsed_time(e))
        print(f"  {what} alone {sum(part) / len(part):.3f} ms  (min {min(part):.3f}, max {max(part):.3f} of {len(part)})")
name = (f"teacher_lse+ce_fwd_kl({args.kl:g})" if args.kl is not None else "ce_fwd_metrics" if args.metrics else f"ce_fwd_smooth({args.smooth:g}, z {args.z or 0.0:g})" if args.smooth is not None
        else "ce_fwd" if args.z is None else f"ce_fwd_z({args.z:g})")
print(f"{name} {mean:.3f} ms  (min {min(ms):.3f}, max {max(ms):.3f} of {len(ms)}; {3 * T * LD * 2 / mean / 1e9:.2f} TB/s at 3 passes, "
      f"{2 * T * LD * 2 / mean / 1e9:.2f} at 2)  loss {float(row_loss.sum()):.4f}" + ("" if args.z is None or args.metrics else f"  z {float(row_z.sum()):.4f}")
      + ("" if args.smooth is None or args.metrics else f"  u {float(row_u.sum()):.4f}") + ("" if args.kl is None else f"  kl {float(row_kl.sum()):.4f}") + (f"  top-1 {int((row_rank == 0).sum())}" if args.metrics else ""))
