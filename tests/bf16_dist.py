"""Distance between a bf16 result and a bf16 reference of the same operation, for the parity tests of the element-wise kernels."""
import torch


def bf16_spacing(ref: torch.Tensor) -> torch.Tensor:
    """fp64 spacing of the bf16 grid at ``|ref|`` (the step to the next larger magnitude): ``2**(e - 7)`` for ``2**e <= |ref| < 2**(e + 1)``;
    ``2**-133`` (the smallest bf16 subnormal) at zero and among the subnormals."""
    r = ref.double().abs()
    _, e = torch.frexp(r)            # r = f * 2**e, f in [0.5, 1)
    sp = torch.ldexp(torch.ones_like(r), (e - 8).to(torch.int32))
    return torch.where(r >= 2.0 ** -126, sp, torch.full_like(r, 2.0 ** -133))


def bf16_distance(x: torch.Tensor, ref: torch.Tensor, floor=0.0) -> tuple[float, float]:
    """``(fraction bit-equal, largest distance in bf16 steps)`` of ``x`` against ``ref`` (both bf16, same shape, finite).

    Bit-equal compares the 16-bit patterns (so +0 and -0 differ).  The distance of one element is ``|x - ref| / max(spacing(ref), floor)``,
    taken in fp64 (exact for bf16 operands): ``spacing`` as in :func:`bf16_spacing`.  Near zero a step of the reference's own grid means
    nothing — an AdamW update of size ``lr`` can carry a weight across zero, where the grid is finer than any rounding of the update — so the
    caller passes ``floor``, an absolute step (a number or a tensor broadcast against ``ref``) below which the grid is not refined: for a
    weight, ``lr * 2**-7``, one bf16 step of the update itself; for a first moment, ``(1 - beta1) * max|g| * 2**-7`` over the steps so far,
    one step of the largest term the updates added (m itself can cancel to near zero).  With ``floor = 0`` the distance is in steps of the
    reference's grid everywhere."""
    assert x.dtype == ref.dtype == torch.bfloat16 and x.shape == ref.shape
    x, ref = x.detach().cpu(), ref.detach().cpu()
    if x.numel() == 0:
        return 1.0, 0.0
    eq = float((x.view(torch.int16) == ref.view(torch.int16)).double().mean())
    fl = floor.detach().cpu().double() if torch.is_tensor(floor) else torch.tensor(float(floor), dtype=torch.float64)
    step = torch.maximum(bf16_spacing(ref), fl)
    d = (x.double() - ref.double()).abs() / step
    return eq, float(d.max())
