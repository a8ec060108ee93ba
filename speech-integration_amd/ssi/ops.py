"""Tensor-level wrappers over the C ABI (``include/ssi_hip.h``).  Thin by design: shape checks on the host, raw device
pointers and the current HIP stream across the ABI, no torch compute ops.  Every function raises on failure."""

from __future__ import annotations

import torch
from typing import Optional
from torch import Tensor

from . import _lib
from ._lib import GEMM_NN, GEMM_NT, GEMM_TN, check, dtype_code, ptr, stream_ptr

__all__ = ["gemm_skinny", "gemm_skinny_rope", "gemm_skinny_swiglu", "weight_quant_fp8", "gemm_skinny_w8", "gemm_skinny_rope_w8", "gemm_skinny_swiglu_w8", "lmhead_ce_fwd", "lmhead_ce_bwd", "doc_ranges", "embed_fwd", "embed_bwd", "rmsnorm_fwd", "rmsnorm_bwd", "rope_", "attn_fwd", "attn_bwd", "attn_bwd_workspace_bytes", "kv_store", "attn_decode", "attn_decode_beam", "attn_decode_split", "attn_decode_beam_split", "attn_decode_split_span", "attn_decode_split_workspace", "decode_select", "decode_sample", "decode_select_pen", "decode_sample_pen", "decode_penalty_lds_bytes", "topk_logprob", "swiglu_fwd",
           "swiglu_bwd", "gemm", "gemm_splitk", "splitk_choice", "gemm_swiglu_fwd", "gemm_swiglu_bwd", "transpose", "ce_fwd", "ce_fwd_z", "ce_fwd_smooth", "ce_fwd_kl", "ce_reduce", "ce_fwd_metrics", "ce_metrics_reduce", "seq_score_reduce", "edit_distance", "bpe_pair_count", "bpe_train_workspace_bytes", "bpe_train_begin", "bpe_merge", "bpe_encode", "count_tokens", "scale_", "sumsq", "adamw_step", "adamw_step_seg", "round_bf16_sr", "ema_update", "set_impl", "set_attn_impl", "attn_last_dispatch",
           "kv_store_fp8", "attn_decode_fp8", "attn_decode_beam_fp8", "attn_decode_split_fp8", "attn_decode_beam_split_fp8",
           "GEMM_NT", "GEMM_NN", "GEMM_TN"]


def set_impl(impl: int) -> int:
    return _lib.load().ssi_set_impl(impl)


def set_attn_impl(which: int, mode: int) -> int:
    """Which attention backward kernels may run (``_lib.ATTN_KERNEL_*`` x ``_lib.ATTN_MODE_*``; process-global); returns the previous mode."""
    return _lib.load().ssi_set_attn_impl(which, mode)


def attn_last_dispatch() -> int:
    """Bit set of ``_lib.ATTN_USED_*``: the kernels the most recent MFMA attention backward of the process launched."""
    return _lib.load().ssi_attn_last_dispatch()


def _byte_ws(nbytes: int, like: Tensor) -> Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=like.device)


def embed_fwd(tokens: Tensor, table: Tensor, out: Tensor, vocab: int) -> None:
    n, dim = tokens.numel(), table.shape[1]
    assert tokens.dtype == torch.int64 and tokens.is_contiguous() and out.is_contiguous() and table.stride(1) == 1
    assert table.stride(0) == dim and out.shape[-1] == dim and out.numel() == n * dim and out.dtype == table.dtype
    check(_lib.load().ssi_embed_fwd(ptr(tokens), ptr(table), ptr(out), n, dim, vocab, dtype_code(table.dtype),
                                    stream_ptr()), "ssi_embed_fwd")


def embed_bwd(tokens: Tensor, dout: Tensor, dtable: Tensor, vocab: int, workspace: Tensor | None = None) -> None:
    lib = _lib.load()
    n, dim = tokens.numel(), dtable.shape[1]
    assert tokens.dtype == torch.int64 and tokens.is_contiguous() and dout.is_contiguous() and dtable.stride(0) == dim
    need = lib.ssi_embed_bwd_workspace_bytes(vocab)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = _byte_ws(need, dout)
    check(lib.ssi_embed_bwd(ptr(tokens), ptr(dout), ptr(dtable), n, dim, vocab, dtype_code(dtable.dtype), ptr(workspace),
                            workspace.numel() * workspace.element_size(), stream_ptr()), "ssi_embed_bwd")


def rmsnorm_fwd(x: Tensor, scale: Tensor, y: Tensor, rstd: Tensor | None, eps: float) -> None:
    dim = x.shape[-1]
    rows = x.numel() // dim
    assert x.is_contiguous() and y.is_contiguous() and scale.is_contiguous() and scale.numel() == dim
    assert rstd is None or (rstd.dtype == torch.float32 and rstd.numel() >= rows)
    check(_lib.load().ssi_rmsnorm_fwd(ptr(x), ptr(scale), ptr(y), ptr(rstd), rows, dim, eps, dtype_code(x.dtype),
                                      stream_ptr()), "ssi_rmsnorm_fwd")


def rmsnorm_bwd_workspace_bytes(rows: int, dim: int) -> int:
    return _lib.load().ssi_rmsnorm_bwd_workspace_bytes(rows, dim)


def rmsnorm_bwd(dy: Tensor, x: Tensor, scale: Tensor, rstd: Tensor, dres: Tensor | None, dx: Tensor, dscale: Tensor,
                workspace: Tensor | None = None, accumulate: bool = True) -> None:
    lib = _lib.load()
    dim = x.shape[-1]
    rows = x.numel() // dim
    assert dy.is_contiguous() and x.is_contiguous() and dx.is_contiguous() and dscale.is_contiguous()
    assert dres is None or dres.is_contiguous()
    need = lib.ssi_rmsnorm_bwd_workspace_bytes(rows, dim)
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = _byte_ws(need, dy)
    check(lib.ssi_rmsnorm_bwd(ptr(dy), ptr(x), ptr(scale), ptr(rstd), ptr(dres), ptr(dx), ptr(dscale), int(accumulate), rows, dim,
                              dtype_code(x.dtype), ptr(workspace), workspace.numel() * workspace.element_size(),
                              stream_ptr()), "ssi_rmsnorm_bwd")


def rope_(x: Tensor, seq_len: int, n_heads_rot: int, head_dim: int, table: Tensor, inverse: bool = False,
          positions: Tensor | None = None) -> None:
    """In-place rotation of the first ``n_heads_rot`` heads of each row of ``x`` ([rows, ld])."""
    assert x.dim() == 2 and x.stride(1) == 1 and table.dtype == torch.float32 and table.is_contiguous()
    assert positions is None or (positions.dtype == torch.int32 and positions.numel() == x.shape[0])
    check(_lib.load().ssi_rope_inplace(ptr(x), x.stride(0), x.shape[0], seq_len, n_heads_rot, head_dim, ptr(table),
                                       table.shape[0], ptr(positions), int(inverse), dtype_code(x.dtype), stream_ptr()),
          "ssi_rope_inplace")


def gemm_rope(a: Tensor, b: Tensor, c: Tensor, seq_len: int, n_heads_rot: int, head_dim: int, table: Tensor,
              positions: Tensor | None = None) -> None:
    """c = a @ b^T, then ``rope_`` on the first ``n_heads_rot`` heads of every row of c (QKV projection + RoPE, one launch on the
    MFMA path)."""
    assert a.dim() == 2 and b.dim() == 2 and c.dim() == 2 and a.stride(1) == 1 and b.stride(1) == 1 and c.stride(1) == 1
    M, K = a.shape
    N = b.shape[0]
    assert b.shape[1] == K and c.shape == (M, N) and a.dtype == b.dtype == c.dtype
    assert table.dtype == torch.float32 and table.is_contiguous() and table.shape[1] * 2 == head_dim
    assert positions is None or (positions.dtype == torch.int32 and positions.numel() == M)
    check(_lib.load().ssi_gemm_rope(M, N, K, ptr(a), a.stride(0), ptr(b), b.stride(0), ptr(c), c.stride(0), seq_len, n_heads_rot, head_dim,
                                    ptr(table), table.shape[0], ptr(positions), dtype_code(a.dtype), stream_ptr()), "ssi_gemm_rope")


def _doc_ptrs(doc_start: Optional[Tensor], doc_end: Optional[Tensor], rows: int):
    if doc_start is None and doc_end is None:
        return None, None
    assert doc_start is not None and doc_end is not None, "doc_start and doc_end go together"
    for t in (doc_start, doc_end):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == rows
    return ptr(doc_start), ptr(doc_end)


def doc_ranges(input_pos: Tensor, max_pos: int, n_clamped: Tensor | None = None) -> tuple[Tensor, Tensor, Tensor]:
    """Packed rows: int32 [B*S] (positions clamped to max_pos, doc_start, doc_end) from input_pos [B, S] in one launch.  ``n_clamped``
    (int32 [1], zeroed by the caller) receives the number of positions that had to be clamped."""
    assert input_pos.dim() == 2 and input_pos.dtype == torch.int64
    assert n_clamped is None or (n_clamped.dtype == torch.int32 and n_clamped.numel() == 1)
    ip = input_pos.contiguous()
    B, S = ip.shape
    out = torch.empty(3, B * S, dtype=torch.int32, device=ip.device)
    check(_lib.load().ssi_doc_ranges(ptr(ip), B, S, int(max_pos), ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(n_clamped), stream_ptr()),
          "ssi_doc_ranges")
    return out[0], out[1], out[2]


def set_gemm_tile_order(dynamic: bool) -> None:
    """Dynamic tile order for the persistent GEMMs (use when other kernels share the GPU, e.g. RCCL during backward)."""
    check(_lib.load().ssi_set_gemm_tile_order(_lib.TILES_DYNAMIC if dynamic else _lib.TILES_STATIC), "ssi_set_gemm_tile_order")


def attn_fwd(qkv: Tensor, out: Tensor, lse: Tensor, batch: int, seq: int, n_heads: int, n_kv: int, head_dim: int,
             doc_start: Optional[Tensor] = None, doc_end: Optional[Tensor] = None) -> None:
    """Causal GQA attention; with doc_start / doc_end (int32 [batch*seq]) block-causal over the documents packed in a row."""
    assert qkv.dim() == 2 and qkv.stride(1) == 1 and out.is_contiguous() and lse.dtype == torch.float32
    assert qkv.shape[0] == batch * seq and out.numel() == batch * seq * n_heads * head_dim
    assert lse.numel() >= batch * n_heads * seq
    ds, de = _doc_ptrs(doc_start, doc_end, batch * seq)
    check(_lib.load().ssi_attn_varlen_fwd(ptr(qkv), qkv.stride(0), ptr(out), ptr(lse), ds, de, batch, seq, n_heads, n_kv, head_dim,
                                          dtype_code(qkv.dtype), stream_ptr()), "ssi_attn_varlen_fwd")


def attn_bwd_workspace_bytes(batch: int, seq: int, n_heads: int, n_kv: int, head_dim: int, dtype: torch.dtype) -> int:
    """Bytes of workspace ``attn_bwd`` can use for this shape (0: none): small launches then run dK / dV per query head + a reduction."""
    return int(_lib.load().ssi_attn_bwd_workspace_bytes(batch, seq, n_heads, n_kv, head_dim, dtype_code(dtype)))


def attn_bwd(qkv: Tensor, out: Tensor, dout: Tensor, lse: Tensor, dqkv: Tensor, delta: Tensor, batch: int, seq: int,
             n_heads: int, n_kv: int, head_dim: int, doc_start: Optional[Tensor] = None, doc_end: Optional[Tensor] = None,
             rope_table: Optional[Tensor] = None, positions: Optional[Tensor] = None, workspace: Optional[Tensor] = None, plan=None) -> None:
    """dqkv of causal (or block-causal) GQA attention.  With ``rope_table`` the q / k parts come back in pre-RoPE space (the
    backward of ``rope_`` fused in), positions as in ``rope_``.  ``workspace`` (bytes, see ``attn_bwd_workspace_bytes``): optional.
    ``plan`` (``ssi.attn_plan.AttnPlan`` on the device, packed rows only): the pipelined kernels take the documents' work from it."""
    assert qkv.stride(1) == 1 and dqkv.stride() == qkv.stride() and out.is_contiguous() and dout.is_contiguous()
    assert delta.dtype == torch.float32 and delta.numel() >= batch * n_heads * seq
    assert workspace is None or (workspace.is_contiguous() and workspace.dtype == torch.uint8)
    assert rope_table is None or (rope_table.dtype == torch.float32 and rope_table.is_contiguous() and rope_table.shape[1] * 2 == head_dim)
    assert positions is None or (positions.dtype == torch.int32 and positions.numel() == batch * seq)
    ds, de = _doc_ptrs(doc_start, doc_end, batch * seq)
    ws_bytes = workspace.numel() if workspace is not None else 0
    table_len = rope_table.shape[0] if rope_table is not None else 0
    plan_dev = plan_header = None
    if plan is not None:
        assert plan.dev is not None and plan.dev.device == qkv.device and plan.matches(batch, seq, n_heads, n_kv)
        assert ds is not None or (positions is None and plan.n_docs == batch), "a plan for plain rows has one document per row"
        if ws_bytes < plan.workspace_bytes:  # fp32 partial rows of the dK/dV chunks the plan splits over the query heads
            workspace = _byte_ws(plan.workspace_bytes, qkv)
            ws_bytes = workspace.numel()
        plan_dev, plan_header = ptr(plan.dev), plan.host.data_ptr()
    # the widest entry; ssi_attn_bwd, ssi_attn_varlen_bwd, _rope and _ws are this one with NULL / 0 for what the caller did not bring
    check(_lib.load().ssi_attn_varlen_bwd_plan(ptr(qkv), qkv.stride(0), ptr(out), ptr(dout), ptr(lse), ptr(dqkv), ptr(delta), ds, de,
                                               ptr(rope_table), table_len, ptr(positions), batch, seq, n_heads, n_kv, head_dim,
                                               dtype_code(qkv.dtype), ptr(workspace), ws_bytes, plan_dev, plan_header, stream_ptr()),
          "ssi_attn_varlen_bwd_plan")


def _kv_cache_ok(k_cache: Tensor, v_cache: Tensor, like: Tensor, n_kv: int, head_dim: int) -> None:
    for c in (k_cache, v_cache):
        if c.dim() != 3 or c.shape[2] != n_kv * head_dim or not c.is_contiguous() or c.dtype != like.dtype or c.device != like.device:
            raise _lib.HipLibraryError(f"a K/V cache is a contiguous [n_slots, cap, {n_kv * head_dim}] tensor of the dtype and device of qkv "
                                       f"(got {tuple(c.shape)}, {c.dtype}, {c.device})")
    if k_cache.shape != v_cache.shape:
        raise _lib.HipLibraryError(f"k_cache {tuple(k_cache.shape)} and v_cache {tuple(v_cache.shape)} differ")


def kv_store(qkv: Tensor, dest: Tensor, k_cache: Tensor, v_cache: Tensor, n_heads: int, n_kv: int, head_dim: int,
             n_bad: Tensor | None = None) -> None:
    """``cache[dest[r]]`` = the k / v columns of row ``r`` of ``qkv`` ([rows, ld], q | k | v heads); the caches are
    ``[n_slots, cap, n_kv * head_dim]`` and ``dest[r] = slot * cap + position`` (int64; -1 skips the row).  A ``dest`` outside the cache is
    skipped and counted into ``n_bad`` (int32 [1], zeroed by the caller).  ``ssi_kv_store``: a bit-exact copy."""
    ptr(qkv)
    if qkv.dim() != 2 or qkv.stride(1) != 1 or qkv.shape[1] < (n_heads + 2 * n_kv) * head_dim:
        raise _lib.HipLibraryError(f"kv_store: qkv must be [rows, >= {(n_heads + 2 * n_kv) * head_dim}] with unit inner stride (got {tuple(qkv.shape)})")
    _kv_cache_ok(k_cache, v_cache, qkv, n_kv, head_dim)
    if dest.dtype != torch.int64 or not dest.is_contiguous() or dest.numel() != qkv.shape[0] or dest.device != qkv.device:
        raise _lib.HipLibraryError("kv_store: dest is one int64 per row of qkv, on its device")
    if n_bad is not None and (n_bad.dtype != torch.int32 or n_bad.numel() != 1 or n_bad.device != qkv.device):
        raise _lib.HipLibraryError("kv_store: n_bad is one int32 on the device of qkv")
    check(_lib.load().ssi_kv_store(ptr(qkv), qkv.stride(0), ptr(dest), qkv.shape[0], k_cache.shape[0] * k_cache.shape[1], ptr(k_cache), ptr(v_cache),
                                   n_heads, n_kv, head_dim, ptr(n_bad), dtype_code(qkv.dtype), stream_ptr()), "ssi_kv_store")


def _kv_fp8_ok(what: str, k_codes: Tensor, v_codes: Tensor, k_exp: Tensor, v_exp: Tensor, like: Tensor, n_kv: int, head_dim: int) -> None:
    """One fp8 cache (the header's "FP8 K/V cache"): codes ``[n_slots, cap, n_kv * head_dim]`` and exponent bytes ``[n_slots, cap, n_kv]``, uint8,
    contiguous, on the device of ``like``; refused before the library is loaded."""
    for name, t, last in (("k_codes", k_codes, n_kv * head_dim), ("v_codes", v_codes, n_kv * head_dim), ("k_exp", k_exp, n_kv), ("v_exp", v_exp, n_kv)):
        if not isinstance(t, Tensor) or t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != last or not t.is_contiguous() or t.device != like.device:
            got = (tuple(t.shape), t.dtype, t.device) if isinstance(t, Tensor) else type(t).__name__
            raise _lib.HipLibraryError(f"{what}: {name} is a contiguous uint8 [n_slots, cap, {last}] tensor on the device of qkv (got {got})")
    if k_codes.shape != v_codes.shape or k_exp.shape != v_exp.shape or k_exp.shape[:2] != k_codes.shape[:2]:
        raise _lib.HipLibraryError(f"{what}: codes {tuple(k_codes.shape)} / {tuple(v_codes.shape)} and exponents {tuple(k_exp.shape)} / "
                                   f"{tuple(v_exp.shape)} are not one cache")


def kv_store_fp8(qkv: Tensor, dest: Tensor, k_codes: Tensor, v_codes: Tensor, k_exp: Tensor, v_exp: Tensor, n_heads: int, n_kv: int, head_dim: int,
                 n_bad: Tensor | None = None) -> None:
    """``kv_store`` into an fp8 cache: every line (one kv head of k or of v of a row) as ``head_dim`` e4m3 codes and one exponent byte, by the
    header's definition; ``dest`` and ``n_bad`` as there.  ``ssi_kv_store_fp8``."""
    if not isinstance(qkv, Tensor) or qkv.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.HipLibraryError("kv_store_fp8: qkv is an fp32 or bf16 tensor")
    _kv_fp8_ok("kv_store_fp8", k_codes, v_codes, k_exp, v_exp, qkv, n_kv, head_dim)
    ptr(qkv)
    if qkv.dim() != 2 or qkv.stride(1) != 1 or qkv.shape[1] < (n_heads + 2 * n_kv) * head_dim:
        raise _lib.HipLibraryError(f"kv_store_fp8: qkv must be [rows, >= {(n_heads + 2 * n_kv) * head_dim}] with unit inner stride (got {tuple(qkv.shape)})")
    if dest.dtype != torch.int64 or not dest.is_contiguous() or dest.numel() != qkv.shape[0] or dest.device != qkv.device:
        raise _lib.HipLibraryError("kv_store_fp8: dest is one int64 per row of qkv, on its device")
    if n_bad is not None and (n_bad.dtype != torch.int32 or n_bad.numel() != 1 or n_bad.device != qkv.device):
        raise _lib.HipLibraryError("kv_store_fp8: n_bad is one int32 on the device of qkv")
    check(_lib.load().ssi_kv_store_fp8(ptr(qkv), qkv.stride(0), ptr(dest), qkv.shape[0], k_codes.shape[0] * k_codes.shape[1], ptr(k_codes), ptr(v_codes),
                                       ptr(k_exp), ptr(v_exp), n_heads, n_kv, head_dim, ptr(n_bad), dtype_code(qkv.dtype), stream_ptr()),
          "ssi_kv_store_fp8")


def _decode_rows(what: str, qkv: Tensor, int32_rows, out: Tensor, lse: Tensor | None, n_heads: int, head_dim: int, n_bad: Tensor | None) -> int:
    """The checks the decode-attention wrappers share, under the wrapper's name ``what``: the q rows, one int32 per row for every ``(name, tensor)``
    of ``int32_rows``, ``out``, ``lse`` and ``n_bad``.  Returns the number of rows."""
    ptr(qkv)
    if qkv.dim() != 2 or qkv.stride(1) != 1 or qkv.shape[1] < n_heads * head_dim:
        raise _lib.HipLibraryError(f"{what}: qkv must be [rows, >= {n_heads * head_dim}] with unit inner stride (got {tuple(qkv.shape)})")
    rows = qkv.shape[0]
    for name, t in int32_rows:
        if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != rows or t.device != qkv.device:
            raise _lib.HipLibraryError(f"{what}: {name} is one int32 per row of qkv, on its device")
    if out.dtype != qkv.dtype or not out.is_contiguous() or out.numel() != rows * n_heads * head_dim or out.device != qkv.device:
        raise _lib.HipLibraryError(f"{what}: out must be a contiguous [rows, {n_heads * head_dim}] tensor of the dtype and device of qkv")
    if lse is not None and (lse.dtype != torch.float32 or not lse.is_contiguous() or lse.numel() < rows * n_heads or lse.device != qkv.device):
        raise _lib.HipLibraryError(f"{what}: lse is fp32 [rows, n_heads] on the device of qkv")
    if n_bad is not None and (n_bad.dtype != torch.int32 or n_bad.numel() != 1 or n_bad.device != qkv.device):
        raise _lib.HipLibraryError(f"{what}: n_bad is one int32 on the device of qkv")
    return rows


def _slot_args(what: str, qkv: Tensor, k_cache: Tensor, v_cache: Tensor, slot: Tensor, kv_len: Tensor, out: Tensor, lse: Tensor | None,
               n_heads: int, n_kv: int, head_dim: int, n_bad: Tensor | None) -> tuple:
    """Checks and leading C arguments of ``attn_decode`` and its split form (up to ``n_bad``)."""
    rows = _decode_rows(what, qkv, (("slot", slot), ("kv_len", kv_len)), out, lse, n_heads, head_dim, n_bad)
    _kv_cache_ok(k_cache, v_cache, qkv, n_kv, head_dim)
    return (ptr(qkv), qkv.stride(0), ptr(k_cache), ptr(v_cache), k_cache.shape[0], k_cache.shape[1], ptr(slot), ptr(kv_len), ptr(out), ptr(lse),
            rows, n_heads, n_kv, head_dim, ptr(n_bad))


def _beam_args(what: str, qkv: Tensor, pk_cache: Tensor, pv_cache: Tensor, bk_cache: Tensor, bv_cache: Tensor, prompt_slot: Tensor,
               prompt_len: Tensor, gen_len: Tensor, anc: Tensor, out: Tensor, lse: Tensor | None, n_heads: int, n_kv: int, head_dim: int,
               n_bad: Tensor | None) -> tuple:
    """Checks and leading C arguments of ``attn_decode_beam`` and its split form (up to ``n_bad``)."""
    rows = _decode_rows(what, qkv, (("prompt_slot", prompt_slot), ("prompt_len", prompt_len), ("gen_len", gen_len)), out, lse, n_heads, head_dim, n_bad)
    _kv_cache_ok(pk_cache, pv_cache, qkv, n_kv, head_dim)
    _kv_cache_ok(bk_cache, bv_cache, qkv, n_kv, head_dim)
    if anc.dtype != torch.int32 or anc.dim() != 2 or anc.shape[0] != rows or not anc.is_contiguous() or anc.device != qkv.device:
        raise _lib.HipLibraryError(f"{what}: anc is a contiguous int32 [rows, ld_anc] tensor on the device of qkv")
    return (ptr(qkv), qkv.stride(0), ptr(pk_cache), ptr(pv_cache), pk_cache.shape[0], pk_cache.shape[1], ptr(bk_cache), ptr(bv_cache),
            bk_cache.shape[0], bk_cache.shape[1], ptr(prompt_slot), ptr(prompt_len), ptr(gen_len), ptr(anc), anc.shape[1], ptr(out), ptr(lse),
            rows, n_heads, n_kv, head_dim, ptr(n_bad))


def _split_workspace(what: str, qkv: Tensor, workspace: Tensor, span: int) -> None:
    """What a split wrapper refuses before anything else (and before the library is loaded): a workspace that is no contiguous fp32 tensor on the
    device of ``qkv``, a span that is no positive integer."""
    if not isinstance(workspace, Tensor) or workspace.dtype != torch.float32 or not workspace.is_contiguous() or workspace.device != qkv.device:
        raise _lib.HipLibraryError(f"{what}: workspace is a contiguous fp32 tensor on the device of qkv")
    if int(span) != span or span < 1:
        raise _lib.HipLibraryError(f"{what}: span is a positive number of keys (got {span})")


def attn_decode_split_span(head_dim: int, dtype: torch.dtype) -> int:
    """The library's default span in keys for this head width and storage type (``ssi_attn_decode_split_span``); 0: unsupported."""
    return int(_lib.load().ssi_attn_decode_split_span(int(head_dim), dtype_code(dtype)))


def attn_decode_split_workspace(rows: int, n_heads: int, head_dim: int, keys: int, span: int) -> int:
    """fp32 ELEMENTS of the workspace of a split launch of ``rows`` rows whose caches hold up to ``keys`` keys per row."""
    return int(_lib.load().ssi_attn_decode_split_workspace(int(rows), int(n_heads), int(head_dim), max(_cdiv(int(keys), int(span)), 1))) // 4


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def attn_decode(qkv: Tensor, k_cache: Tensor, v_cache: Tensor, slot: Tensor, kv_len: Tensor, out: Tensor, lse: Tensor | None, n_heads: int,
                n_kv: int, head_dim: int, n_bad: Tensor | None = None) -> None:
    """Single-query GQA attention of row ``r`` of ``qkv`` (its q heads) over the first ``kv_len[r]`` cached keys of slot ``slot[r]`` (int32
    each): ``out`` [rows, n_heads * head_dim], ``lse`` (fp32 [rows, n_heads], optional).  ``slot < 0`` or ``kv_len <= 0``: a zero row;
    ``slot >= n_slots``: a zero row, counted into ``n_bad`` (int32 [1]).  ``ssi_attn_decode``: fp32 throughout, one rounding on the store."""
    args = _slot_args("attn_decode", qkv, k_cache, v_cache, slot, kv_len, out, lse, n_heads, n_kv, head_dim, n_bad)
    check(_lib.load().ssi_attn_decode(*args, dtype_code(qkv.dtype), stream_ptr()), "ssi_attn_decode")


def attn_decode_split(qkv: Tensor, k_cache: Tensor, v_cache: Tensor, slot: Tensor, kv_len: Tensor, out: Tensor, lse: Tensor | None, n_heads: int,
                      n_kv: int, head_dim: int, *, span: int, workspace: Tensor, n_bad: Tensor | None = None) -> None:
    """``attn_decode`` with the keys of every (row, kv head) split into spans of ``span`` keys (a positive multiple of the form's round,
    ``8 x`` the keys per load), one workgroup each, and a merge launch behind them (the header's definition).  ``n_splits = ceil(cap / span)``;
    ``workspace``: fp32, at least ``attn_decode_split_workspace(rows, n_heads, head_dim, cap, span)`` elements, never zeroed.  A row with
    ``kv_len <= span`` equals ``attn_decode`` by value; a row's result depends on its own inputs and ``span`` only.  ``ssi_attn_decode_split``."""
    _split_workspace("attn_decode_split", qkv, workspace, span)
    args = _slot_args("attn_decode_split", qkv, k_cache, v_cache, slot, kv_len, out, lse, n_heads, n_kv, head_dim, n_bad)
    check(_lib.load().ssi_attn_decode_split(*args, int(span), max(_cdiv(k_cache.shape[1], int(span)), 1), ptr(workspace), workspace.numel() * 4,
                                            dtype_code(qkv.dtype), stream_ptr()), "ssi_attn_decode_split")


def _selection_rows(what: str, logits: Tensor, vocab: int, token: Tensor, logprob: Tensor | None, int32_rows, allow: Tensor | None,
                    allow_early: Tensor | None) -> int:
    """The checks the four selection wrappers share, under the wrapper's name ``what``: the logits, one entry per row of ``token`` (int64),
    ``logprob`` (fp32) and every ``(name, tensor)`` of ``int32_rows``, and the two bit masks.  Returns the number of rows."""
    ptr(logits)
    if logits.dim() != 2 or logits.stride(1) != 1 or not 1 <= vocab <= logits.shape[1]:
        raise _lib.HipLibraryError(f"{what}: logits must be [rows, >= vocab] with unit inner stride (got {tuple(logits.shape)}, vocab {vocab})")
    rows, words = logits.shape[0], (vocab + 31) // 32
    for name, t, dtype in (("token", token, torch.int64), ("logprob", logprob, torch.float32), *((name, t, torch.int32) for name, t in int32_rows)):
        if t is not None and (t.dtype != dtype or not t.is_contiguous() or t.numel() != rows or t.device != logits.device):
            raise _lib.HipLibraryError(f"{what}: {name} is one {dtype} per row of logits, on its device")
    for name, t in (("allow", allow), ("allow_early", allow_early)):
        if t is not None and (t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != words or t.device != logits.device):
            raise _lib.HipLibraryError(f"{what}: {name} is {words} int32 words (one bit per column) on the device of logits")
    return rows


def _draw_args(what: str, seed: int, step: int, top_k: int) -> int:
    """The ranges of ``seed`` and ``step`` the two sampling wrappers share; returns ``top_k`` as the C entry takes it."""
    if not 0 <= int(seed) < 2 ** 64 or not 0 <= int(step) < 2 ** 32:
        raise _lib.HipLibraryError(f"{what}: seed is in [0, 2^64) and step in [0, 2^32) (got {seed}, {step})")
    return max(-1, min(int(top_k), 2 ** 62))


def decode_select(logits: Tensor, vocab: int, token: Tensor, logprob: Tensor | None = None, rank: Tensor | None = None, *,
                  allow: Tensor | None = None, allow_early: Tensor | None = None, n_generated: Tensor | None = None, min_new: int = 0) -> None:
    """The constrained greedy token of every row of ``logits`` ([rows, ld], unit inner stride; read only): ``token`` (int64) = the first
    allowed column below ``vocab`` that holds the maximum over the allowed columns, ``logprob`` (fp32, optional) = its log-probability over ALL
    real columns, ``rank`` (int32, optional) = its position in a stable descending sort of the row (0: the constraint did not bind).  ``allow``
    / ``allow_early``: int32 bit masks of ``ceil(vocab / 32)`` words (bit ``c % 32`` of word ``c // 32``), ``None`` = every column; row ``r``
    takes ``allow_early`` while ``n_generated[r] < min_new`` (int32 per row).  A row with nothing allowed: -1 / 0 / -1.  ``ssi_decode_select``."""
    rows = _selection_rows("decode_select", logits, vocab, token, logprob, (("rank", rank), ("n_generated", n_generated)), allow, allow_early)
    check(_lib.load().ssi_decode_select(ptr(logits), logits.stride(0), rows, int(vocab), ptr(allow), ptr(allow_early), ptr(n_generated),
                                        int(min_new), ptr(token), ptr(logprob), ptr(rank), dtype_code(logits.dtype), stream_ptr()),
          "ssi_decode_select")


def decode_sample(logits: Tensor, vocab: int, token: Tensor, logprob: Tensor | None = None, n_kept: Tensor | None = None, *, temperature: float,
                  top_k: int = -1, top_p: float = 1.0, seed: int, step: int, sequence: Tensor, allow: Tensor | None = None,
                  allow_early: Tensor | None = None, n_generated: Tensor | None = None, min_new: int = 0) -> None:
    """The sampled token of every row of ``logits`` ([rows, ld], unit inner stride; read only): ``token`` (int64) = a draw from
    ``softmax(x / temperature)`` over the allowed columns below ``vocab`` that top-k (``top_k <= 0``: off; ties at the threshold stay) and then
    top-p (``top_p = 1``: off) keep, by Gumbel-max on Philox bits keyed by ``(seed, sequence[r], step)`` — a pure function of those and the row;
    ``logprob`` (fp32, optional) = the token's log-probability over ALL real columns at temperature 1 (``decode_select``'s); ``n_kept`` (int32,
    optional) = the size of the set drawn from.  ``sequence``: one int32 per row, read as unsigned.  The masks, ``n_generated`` and ``min_new``
    are ``decode_select``'s.  A row with nothing allowed: -1 / 0 / -1.  ``ssi_decode_sample``."""
    rows = _selection_rows("decode_sample", logits, vocab, token, logprob, (("n_kept", n_kept), ("n_generated", n_generated), ("sequence", sequence)), allow, allow_early)
    top_k = _draw_args("decode_sample", seed, step, top_k)
    check(_lib.load().ssi_decode_sample(ptr(logits), logits.stride(0), rows, int(vocab), ptr(allow), ptr(allow_early), ptr(n_generated),
                                        int(min_new), float(temperature), top_k, float(top_p), int(seed), int(step), ptr(sequence), ptr(token),
                                        ptr(logprob), ptr(n_kept), dtype_code(logits.dtype), stream_ptr()), "ssi_decode_sample")


def decode_penalty_lds_bytes(vocab: int, ld_gen: int) -> int:
    """The dynamic LDS a penalised selection launch needs: ``4 ceil(vocab / 32) + 8 Hs`` bytes, ``Hs`` the smallest power of two ``>= 2 ld_gen``
    and ``>= 64`` (the header's formula).  A launch is refused above ``_lib.DECODE_PENALTY_LDS_MAX``."""
    hs = 64
    while hs < 2 * int(ld_gen):
        hs *= 2
    return 4 * ((int(vocab) + 31) // 32) + 8 * hs


def _penalty_args(what: str, logits: Tensor, vocab: int, n_generated: Tensor | None, prompt_ids: Tensor | None, prompt_len: Tensor,
                  prompt_row: Tensor | None, gen_ids: Tensor | None, repetition_penalty: float, frequency_penalty: float, presence_penalty: float,
                  n_bad: Tensor | None):
    """The checks and the trailing C arguments the two penalised wrappers share."""
    rows, dev = logits.shape[0], logits.device
    if n_generated is None:
        raise _lib.HipLibraryError(f"{what}: n_generated is required (how many of a row's gen_ids count)")
    if prompt_ids is not None and (prompt_ids.dtype != torch.int32 or prompt_ids.dim() != 2 or not prompt_ids.is_contiguous() or prompt_ids.device != dev):
        raise _lib.HipLibraryError(f"{what}: prompt_ids is a contiguous int32 [n_prompts, ld_prompt] on the device of logits")
    n_prompts = prompt_ids.shape[0] if prompt_ids is not None else prompt_len.numel()
    ld_prompt = prompt_ids.shape[1] if prompt_ids is not None else 0
    if prompt_len.dtype != torch.int32 or not prompt_len.is_contiguous() or prompt_len.numel() != n_prompts or prompt_len.device != dev:
        raise _lib.HipLibraryError(f"{what}: prompt_len is one int32 per line of prompt_ids, on the device of logits")
    if prompt_row is None and n_prompts != rows:
        raise _lib.HipLibraryError(f"{what}: without prompt_row there is one prompt line per row ({n_prompts} lines, {rows} rows)")
    if prompt_row is not None and (prompt_row.dtype != torch.int32 or not prompt_row.is_contiguous() or prompt_row.numel() != rows or prompt_row.device != dev):
        raise _lib.HipLibraryError(f"{what}: prompt_row is one int32 per row of logits, on its device")
    if gen_ids is not None and (gen_ids.dtype != torch.int64 or gen_ids.dim() != 2 or gen_ids.shape[0] != rows or gen_ids.stride(1) != 1
                                or gen_ids.stride(0) < gen_ids.shape[1] or gen_ids.device != dev):
        raise _lib.HipLibraryError(f"{what}: gen_ids is int64 [rows, ld_gen] with unit inner stride, on the device of logits")
    if gen_ids is not None and gen_ids.shape[1] != gen_ids.stride(0) and rows > 1:
        raise _lib.HipLibraryError(f"{what}: gen_ids must be contiguous (row stride {gen_ids.stride(0)} for {gen_ids.shape[1]} columns)")
    ld_gen = gen_ids.shape[1] if gen_ids is not None else 0
    if n_bad is not None and (n_bad.dtype != torch.int32 or n_bad.numel() != 1 or n_bad.device != dev):
        raise _lib.HipLibraryError(f"{what}: n_bad is one int32 on the device of logits")
    need = decode_penalty_lds_bytes(vocab, ld_gen)
    if need > _lib.DECODE_PENALTY_LDS_MAX:
        raise _lib.HipLibraryError(f"{what}: vocab {vocab} with ld_gen {ld_gen} needs {need} bytes of LDS; at most {_lib.DECODE_PENALTY_LDS_MAX}")
    return (ptr(prompt_ids), ld_prompt, ptr(prompt_len), ptr(prompt_row), n_prompts, ptr(gen_ids), ld_gen, float(repetition_penalty),
            float(frequency_penalty), float(presence_penalty), ptr(n_bad))


def decode_select_pen(logits: Tensor, vocab: int, token: Tensor, logprob: Tensor | None = None, rank: Tensor | None = None, *,
                      prompt_ids: Tensor | None, prompt_len: Tensor, prompt_row: Tensor | None = None, gen_ids: Tensor | None,
                      n_generated: Tensor, repetition_penalty: float = 1.0, frequency_penalty: float = 0.0, presence_penalty: float = 0.0,
                      n_bad: Tensor | None = None, allow: Tensor | None = None, allow_early: Tensor | None = None, min_new: int = 0) -> None:
    """``decode_select`` under vLLM's penalties: the token is the first allowed maximum of the PENALISED row ``y`` (the header's definition:
    ``y = fma(x, a, -t)`` on the columns of the row's history, ``x`` elsewhere), ``logprob`` and ``rank`` stay those of the raw row, so ``rank``
    is 0 exactly when neither the mask nor the penalties changed the choice.  History: ``prompt_ids`` int32 ``[n_prompts, ld_prompt]`` with
    ``prompt_len`` per line, row ``r`` reading line ``prompt_row[r]`` (``None``: line ``r``); ``gen_ids`` int64 ``[rows, ld_gen]`` of which row
    ``r`` reads its first ``n_generated[r]`` entries (int32, required).  ``n_bad`` (int32 ``[1]``, optional) counts the rows that held an id or a
    line out of range, which are skipped.  ``ssi_decode_select_pen``."""
    rows = _selection_rows("decode_select_pen", logits, vocab, token, logprob, (("rank", rank), ("n_generated", n_generated)), allow, allow_early)
    tail = _penalty_args("decode_select_pen", logits, int(vocab), n_generated, prompt_ids, prompt_len, prompt_row, gen_ids, repetition_penalty,
                         frequency_penalty, presence_penalty, n_bad)
    check(_lib.load().ssi_decode_select_pen(ptr(logits), logits.stride(0), rows, int(vocab), ptr(allow), ptr(allow_early), ptr(n_generated),
                                            int(min_new), ptr(token), ptr(logprob), ptr(rank), *tail, dtype_code(logits.dtype), stream_ptr()),
          "ssi_decode_select_pen")


def decode_sample_pen(logits: Tensor, vocab: int, token: Tensor, logprob: Tensor | None = None, n_kept: Tensor | None = None, *, temperature: float,
                      top_k: int = -1, top_p: float = 1.0, seed: int, step: int, sequence: Tensor, prompt_ids: Tensor | None, prompt_len: Tensor,
                      prompt_row: Tensor | None = None, gen_ids: Tensor | None, n_generated: Tensor, repetition_penalty: float = 1.0,
                      frequency_penalty: float = 0.0, presence_penalty: float = 0.0, n_bad: Tensor | None = None, allow: Tensor | None = None,
                      allow_early: Tensor | None = None, min_new: int = 0) -> None:
    """``decode_sample`` under vLLM's penalties: the allowed set, top-k, top-p, the masses and the Gumbel-max score are all taken on the
    PENALISED row ``y`` (penalties before temperature: vLLM's order); ``logprob`` stays that of the raw row at temperature 1.  The random bits
    are ``decode_sample``'s.  The history arguments are ``decode_select_pen``'s.  ``ssi_decode_sample_pen``."""
    rows = _selection_rows("decode_sample_pen", logits, vocab, token, logprob, (("n_kept", n_kept), ("n_generated", n_generated), ("sequence", sequence)), allow, allow_early)
    top_k = _draw_args("decode_sample_pen", seed, step, top_k)
    tail = _penalty_args("decode_sample_pen", logits, int(vocab), n_generated, prompt_ids, prompt_len, prompt_row, gen_ids, repetition_penalty,
                         frequency_penalty, presence_penalty, n_bad)
    check(_lib.load().ssi_decode_sample_pen(ptr(logits), logits.stride(0), rows, int(vocab), ptr(allow), ptr(allow_early), ptr(n_generated),
                                            int(min_new), float(temperature), top_k, float(top_p), int(seed), int(step), ptr(sequence), ptr(token),
                                            ptr(logprob), ptr(n_kept), *tail, dtype_code(logits.dtype), stream_ptr()), "ssi_decode_sample_pen")


def _row_draw_args(what: str, logits: Tensor, seed: int, step: Tensor, temperature, top_k, top_p):
    """The draw arguments of the two ``_rows`` wrappers as the C entries take them: the three scalars (a neutral one where a tensor stands for
    it, which the entry then does not read), ``seed``, and the four array pointers.  ``step``: int32 per row, read as unsigned; a tensor for
    ``temperature`` / ``top_p`` is float64 per row, for ``top_k`` int64 per row; a number is the scalar for all rows."""
    rows, dev = logits.shape[0], logits.device
    if not 0 <= int(seed) < 2 ** 64:
        raise _lib.HipLibraryError(f"{what}: seed is in [0, 2^64) (got {seed})")
    scalars, ptrs = [], []
    for name, v, dtype, neutral in (("step", step, torch.int32, None), ("temperature", temperature, torch.float64, 1.0),
                                    ("top_k", top_k, torch.int64, -1), ("top_p", top_p, torch.float64, 1.0)):
        if isinstance(v, Tensor):
            if v.dtype != dtype or not v.is_contiguous() or v.numel() != rows or v.device != dev:
                raise _lib.HipLibraryError(f"{what}: {name} as a tensor is one {dtype} per row of logits, on its device")
            scalars.append(neutral)
            ptrs.append(ptr(v))
        elif neutral is None:
            raise _lib.HipLibraryError(f"{what}: step is an int32 tensor, one entry per row (read as unsigned)")
        else:
            scalars.append(max(-1, min(int(v), 2 ** 62)) if name == "top_k" else float(v))
            ptrs.append(None)
    return (scalars[1], scalars[2], scalars[3], int(seed), *ptrs)


def decode_sample_rows(logits: Tensor, vocab: int, token: Tensor, logprob: Tensor | None = None, n_kept: Tensor | None = None, *,
                       temperature: float | Tensor, top_k: int | Tensor = -1, top_p: float | Tensor = 1.0, seed: int, step: Tensor,
                       sequence: Tensor, allow: Tensor | None = None, allow_early: Tensor | None = None, n_generated: Tensor | None = None,
                       min_new: int = 0) -> None:
    """``decode_sample`` with the step and the draw parameters per row: ``step`` is an int32 tensor (one per row, read as unsigned), and
    ``temperature`` / ``top_p`` (float64) and ``top_k`` (int64) may each be a tensor of one value per row or a number for all rows.  Row ``r``
    has the bits of row ``r`` of ``decode_sample`` launched with its own four values.  A row whose temperature is not finite and > 0, or whose
    ``top_p`` lies outside (0, 1], writes -1 / 0 / -1 and changes no other row.  ``ssi_decode_sample_rows``."""
    rows = _selection_rows("decode_sample_rows", logits, vocab, token, logprob, (("n_kept", n_kept), ("n_generated", n_generated), ("sequence", sequence)), allow, allow_early)
    draw = _row_draw_args("decode_sample_rows", logits, seed, step, temperature, top_k, top_p)
    check(_lib.load().ssi_decode_sample_rows(ptr(logits), logits.stride(0), rows, int(vocab), ptr(allow), ptr(allow_early), ptr(n_generated),
                                             int(min_new), *draw, ptr(sequence), ptr(token), ptr(logprob), ptr(n_kept),
                                             dtype_code(logits.dtype), stream_ptr()), "ssi_decode_sample_rows")


def decode_sample_pen_rows(logits: Tensor, vocab: int, token: Tensor, logprob: Tensor | None = None, n_kept: Tensor | None = None, *,
                           temperature: float | Tensor, top_k: int | Tensor = -1, top_p: float | Tensor = 1.0, seed: int, step: Tensor,
                           sequence: Tensor, prompt_ids: Tensor | None, prompt_len: Tensor, prompt_row: Tensor | None = None,
                           gen_ids: Tensor | None, n_generated: Tensor, repetition_penalty: float = 1.0, frequency_penalty: float = 0.0,
                           presence_penalty: float = 0.0, n_bad: Tensor | None = None, allow: Tensor | None = None,
                           allow_early: Tensor | None = None, min_new: int = 0) -> None:
    """``decode_sample_pen`` with the step and the draw parameters per row (``decode_sample_rows``'s arguments); the penalties stay one
    setting for the launch.  A refused row builds no history and counts nothing into ``n_bad``.  ``ssi_decode_sample_pen_rows``."""
    rows = _selection_rows("decode_sample_pen_rows", logits, vocab, token, logprob, (("n_kept", n_kept), ("n_generated", n_generated), ("sequence", sequence)), allow, allow_early)
    draw = _row_draw_args("decode_sample_pen_rows", logits, seed, step, temperature, top_k, top_p)
    tail = _penalty_args("decode_sample_pen_rows", logits, int(vocab), n_generated, prompt_ids, prompt_len, prompt_row, gen_ids, repetition_penalty,
                         frequency_penalty, presence_penalty, n_bad)
    check(_lib.load().ssi_decode_sample_pen_rows(ptr(logits), logits.stride(0), rows, int(vocab), ptr(allow), ptr(allow_early), ptr(n_generated),
                                                 int(min_new), *draw, ptr(sequence), ptr(token), ptr(logprob), ptr(n_kept), *tail,
                                                 dtype_code(logits.dtype), stream_ptr()), "ssi_decode_sample_pen_rows")


def attn_decode_beam(qkv: Tensor, pk_cache: Tensor, pv_cache: Tensor, bk_cache: Tensor, bv_cache: Tensor, prompt_slot: Tensor, prompt_len: Tensor,
                     gen_len: Tensor, anc: Tensor, out: Tensor, lse: Tensor | None, n_heads: int, n_kv: int, head_dim: int,
                     n_bad: Tensor | None = None) -> None:
    """``attn_decode`` of row ``r`` over two key ranges, one behind the other: the first ``prompt_len[r]`` keys of slot ``prompt_slot[r]`` of the
    prompt cache ``[n_pslots, cap_p, n_kv * head_dim]``, then ``gen_len[r]`` keys of the beam cache ``[n_bslots, cap_b, n_kv * head_dim]``,
    generated position ``i`` from slot ``anc[r, i]`` (int32 ``[rows, ld_anc]``, unit inner stride).  ``prompt_slot < 0``: a zero row.  A
    ``prompt_slot`` or ``anc`` entry outside its cache is never dereferenced: its keys are skipped and the row is counted once into ``n_bad``.
    ``ssi_attn_decode_beam``: bit-equal to ``attn_decode`` on a cache that holds the row's keys contiguously."""
    args = _beam_args("attn_decode_beam", qkv, pk_cache, pv_cache, bk_cache, bv_cache, prompt_slot, prompt_len, gen_len, anc, out, lse, n_heads, n_kv,
                      head_dim, n_bad)
    check(_lib.load().ssi_attn_decode_beam(*args, dtype_code(qkv.dtype), stream_ptr()), "ssi_attn_decode_beam")


def attn_decode_beam_split(qkv: Tensor, pk_cache: Tensor, pv_cache: Tensor, bk_cache: Tensor, bv_cache: Tensor, prompt_slot: Tensor,
                           prompt_len: Tensor, gen_len: Tensor, anc: Tensor, out: Tensor, lse: Tensor | None, n_heads: int, n_kv: int,
                           head_dim: int, *, span: int, workspace: Tensor, n_bad: Tensor | None = None) -> None:
    """``attn_decode_beam`` split as ``attn_decode_split`` splits ``attn_decode``, over the concatenated key index: ``n_splits =
    ceil((cap_p + min(cap_b, ld_anc)) / span)``, the workspace sized for that many keys.  With equal ``span``, equal by value to
    ``attn_decode_split`` on a cache that holds the row's keys contiguously.  ``ssi_attn_decode_beam_split``."""
    _split_workspace("attn_decode_beam_split", qkv, workspace, span)
    args = _beam_args("attn_decode_beam_split", qkv, pk_cache, pv_cache, bk_cache, bv_cache, prompt_slot, prompt_len, gen_len, anc, out, lse, n_heads,
                      n_kv, head_dim, n_bad)
    keys = pk_cache.shape[1] + min(bk_cache.shape[1], anc.shape[1])
    check(_lib.load().ssi_attn_decode_beam_split(*args, int(span), max(_cdiv(keys, int(span)), 1), ptr(workspace), workspace.numel() * 4,
                                                 dtype_code(qkv.dtype), stream_ptr()), "ssi_attn_decode_beam_split")


def _slot_args_fp8(what: str, qkv: Tensor, cache, slot: Tensor, kv_len: Tensor, out: Tensor, lse: Tensor | None, n_heads: int, n_kv: int,
                   head_dim: int, n_bad: Tensor | None) -> tuple:
    """``_slot_args`` for an fp8 cache ``(k_codes, v_codes, k_exp, v_exp)``."""
    if not isinstance(qkv, Tensor) or qkv.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.HipLibraryError(f"{what}: qkv is an fp32 or bf16 tensor")
    _kv_fp8_ok(what, *cache, qkv, n_kv, head_dim)
    rows = _decode_rows(what, qkv, (("slot", slot), ("kv_len", kv_len)), out, lse, n_heads, head_dim, n_bad)
    return (ptr(qkv), qkv.stride(0), *(ptr(t) for t in cache), cache[0].shape[0], cache[0].shape[1], ptr(slot), ptr(kv_len), ptr(out), ptr(lse),
            rows, n_heads, n_kv, head_dim, ptr(n_bad))


def _beam_args_fp8(what: str, qkv: Tensor, pcache, bcache, prompt_slot: Tensor, prompt_len: Tensor, gen_len: Tensor, anc: Tensor, out: Tensor,
                   lse: Tensor | None, n_heads: int, n_kv: int, head_dim: int, n_bad: Tensor | None) -> tuple:
    """``_beam_args`` for an fp8 prompt cache and an fp8 beam cache, each ``(k_codes, v_codes, k_exp, v_exp)``."""
    if not isinstance(qkv, Tensor) or qkv.dtype not in (torch.float32, torch.bfloat16):
        raise _lib.HipLibraryError(f"{what}: qkv is an fp32 or bf16 tensor")
    _kv_fp8_ok(what, *pcache, qkv, n_kv, head_dim)
    _kv_fp8_ok(what, *bcache, qkv, n_kv, head_dim)
    rows = _decode_rows(what, qkv, (("prompt_slot", prompt_slot), ("prompt_len", prompt_len), ("gen_len", gen_len)), out, lse, n_heads, head_dim, n_bad)
    if anc.dtype != torch.int32 or anc.dim() != 2 or anc.shape[0] != rows or not anc.is_contiguous() or anc.device != qkv.device:
        raise _lib.HipLibraryError(f"{what}: anc is a contiguous int32 [rows, ld_anc] tensor on the device of qkv")
    return (ptr(qkv), qkv.stride(0), *(ptr(t) for t in pcache), pcache[0].shape[0], pcache[0].shape[1], *(ptr(t) for t in bcache),
            bcache[0].shape[0], bcache[0].shape[1], ptr(prompt_slot), ptr(prompt_len), ptr(gen_len), ptr(anc), anc.shape[1], ptr(out), ptr(lse),
            rows, n_heads, n_kv, head_dim, ptr(n_bad))


def attn_decode_fp8(qkv: Tensor, k_codes: Tensor, v_codes: Tensor, k_exp: Tensor, v_exp: Tensor, slot: Tensor, kv_len: Tensor, out: Tensor,
                    lse: Tensor | None, n_heads: int, n_kv: int, head_dim: int, n_bad: Tensor | None = None) -> None:
    """``attn_decode`` over an fp8 cache (uint8 codes ``[n_slots, cap, n_kv * head_dim]``, exponent bytes ``[n_slots, cap, n_kv]``).
    ``ssi_attn_decode_fp8``: bit-equal to ``attn_decode`` on a cache that holds the dequantised values in the dtype of ``qkv``."""
    args = _slot_args_fp8("attn_decode_fp8", qkv, (k_codes, v_codes, k_exp, v_exp), slot, kv_len, out, lse, n_heads, n_kv, head_dim, n_bad)
    check(_lib.load().ssi_attn_decode_fp8(*args, dtype_code(qkv.dtype), stream_ptr()), "ssi_attn_decode_fp8")


def attn_decode_split_fp8(qkv: Tensor, k_codes: Tensor, v_codes: Tensor, k_exp: Tensor, v_exp: Tensor, slot: Tensor, kv_len: Tensor, out: Tensor,
                          lse: Tensor | None, n_heads: int, n_kv: int, head_dim: int, *, span: int, workspace: Tensor,
                          n_bad: Tensor | None = None) -> None:
    """``attn_decode_split`` over an fp8 cache; span, splits and workspace as there.  ``ssi_attn_decode_split_fp8``."""
    _split_workspace("attn_decode_split_fp8", qkv, workspace, span)
    args = _slot_args_fp8("attn_decode_split_fp8", qkv, (k_codes, v_codes, k_exp, v_exp), slot, kv_len, out, lse, n_heads, n_kv, head_dim, n_bad)
    check(_lib.load().ssi_attn_decode_split_fp8(*args, int(span), max(_cdiv(k_codes.shape[1], int(span)), 1), ptr(workspace), workspace.numel() * 4,
                                                dtype_code(qkv.dtype), stream_ptr()), "ssi_attn_decode_split_fp8")


def attn_decode_beam_fp8(qkv: Tensor, prompt_cache, beam_cache, prompt_slot: Tensor, prompt_len: Tensor, gen_len: Tensor, anc: Tensor, out: Tensor,
                         lse: Tensor | None, n_heads: int, n_kv: int, head_dim: int, n_bad: Tensor | None = None) -> None:
    """``attn_decode_beam`` over an fp8 prompt cache and an fp8 beam cache, each a ``(k_codes, v_codes, k_exp, v_exp)`` tuple.
    ``ssi_attn_decode_beam_fp8``."""
    args = _beam_args_fp8("attn_decode_beam_fp8", qkv, tuple(prompt_cache), tuple(beam_cache), prompt_slot, prompt_len, gen_len, anc, out, lse,
                          n_heads, n_kv, head_dim, n_bad)
    check(_lib.load().ssi_attn_decode_beam_fp8(*args, dtype_code(qkv.dtype), stream_ptr()), "ssi_attn_decode_beam_fp8")


def attn_decode_beam_split_fp8(qkv: Tensor, prompt_cache, beam_cache, prompt_slot: Tensor, prompt_len: Tensor, gen_len: Tensor, anc: Tensor,
                               out: Tensor, lse: Tensor | None, n_heads: int, n_kv: int, head_dim: int, *, span: int, workspace: Tensor,
                               n_bad: Tensor | None = None) -> None:
    """``attn_decode_beam_split`` over fp8 caches (tuples as in ``attn_decode_beam_fp8``).  ``ssi_attn_decode_beam_split_fp8``."""
    _split_workspace("attn_decode_beam_split_fp8", qkv, workspace, span)
    pc, bc = tuple(prompt_cache), tuple(beam_cache)
    args = _beam_args_fp8("attn_decode_beam_split_fp8", qkv, pc, bc, prompt_slot, prompt_len, gen_len, anc, out, lse, n_heads, n_kv, head_dim, n_bad)
    keys = pc[0].shape[1] + min(bc[0].shape[1], anc.shape[1])
    check(_lib.load().ssi_attn_decode_beam_split_fp8(*args, int(span), max(_cdiv(keys, int(span)), 1), ptr(workspace), workspace.numel() * 4,
                                                     dtype_code(qkv.dtype), stream_ptr()), "ssi_attn_decode_beam_split_fp8")


def topk_logprob(logits: Tensor, vocab: int, k: int, idx: Tensor, lp: Tensor, lse: Tensor | None = None, *, mask: Tensor | None = None) -> None:
    """The ``k`` (1..8) best allowed columns of every row of ``logits`` ([rows, ld], unit inner stride; read only): ``idx`` (int32 ``[rows, k]``)
    by stored value descending, ties to the lower column, NaN below every number, -1 where fewer than ``k`` columns are allowed; ``lp`` (fp32
    ``[rows, k]``) = ``x[idx] - lse``, -inf at -1; ``lse`` (fp32 ``[rows]``, optional) the log-normaliser over ALL real columns ``[0, vocab)``.
    ``mask``: ``decode_select``'s int32 bit mask of ``ceil(vocab / 32)`` words, ``None`` = every column.  ``ssi_topk_logprob``."""
    ptr(logits)
    if logits.dim() != 2 or logits.stride(1) != 1 or not 1 <= vocab <= logits.shape[1]:
        raise _lib.HipLibraryError(f"topk_logprob: logits must be [rows, >= vocab] with unit inner stride (got {tuple(logits.shape)}, vocab {vocab})")
    rows, words, k = logits.shape[0], (vocab + 31) // 32, int(k)
    for name, t, dtype, n in (("idx", idx, torch.int32, rows * k), ("lp", lp, torch.float32, rows * k), ("lse", lse, torch.float32, rows)):
        if t is not None and (t.dtype != dtype or not t.is_contiguous() or t.numel() != n or t.device != logits.device):
            raise _lib.HipLibraryError(f"topk_logprob: {name} is a contiguous {dtype} tensor of {n} elements on the device of logits")
    if mask is not None and (mask.dtype != torch.int32 or not mask.is_contiguous() or mask.numel() != words or mask.device != logits.device):
        raise _lib.HipLibraryError(f"topk_logprob: mask is {words} int32 words (one bit per column) on the device of logits")
    check(_lib.load().ssi_topk_logprob(ptr(logits), logits.stride(0), rows, int(vocab), k, ptr(mask), 0 if mask is None else mask.numel(),
                                       ptr(idx), ptr(lp), ptr(lse), dtype_code(logits.dtype), stream_ptr()), "ssi_topk_logprob")


def swiglu_fwd(gu: Tensor, act: Tensor) -> None:
    inter = act.shape[-1]
    rows = act.numel() // inter
    assert gu.is_contiguous() and act.is_contiguous() and gu.shape[-1] == 2 * inter
    check(_lib.load().ssi_swiglu_fwd(ptr(gu), ptr(act), rows, inter, dtype_code(gu.dtype), stream_ptr()), "ssi_swiglu_fwd")


def swiglu_bwd(dact: Tensor, gu: Tensor, dgu: Tensor) -> None:
    inter = dact.shape[-1]
    rows = dact.numel() // inter
    assert gu.is_contiguous() and dact.is_contiguous() and dgu.is_contiguous() and gu.shape[-1] == 2 * inter
    check(_lib.load().ssi_swiglu_bwd(ptr(dact), ptr(gu), ptr(dgu), rows, inter, dtype_code(gu.dtype), stream_ptr()),
          "ssi_swiglu_bwd")


def gemm(layout: int, a: Tensor, b: Tensor, c: Tensor, *, residual: Tensor | None = None, alpha: float = 1.0,
         alpha_dev: Tensor | None = None, accumulate: bool = False) -> None:
    """c = (accumulate ? c : 0) + alpha * [*alpha_dev] * op(a) op(b) (+ residual).  2-D row-major operands."""
    assert a.dim() == 2 and b.dim() == 2 and c.dim() == 2 and a.stride(1) == 1 and b.stride(1) == 1 and c.stride(1) == 1
    assert a.dtype == b.dtype == c.dtype
    M, N = c.shape
    if layout == GEMM_NT:
        K = a.shape[1]
        assert a.shape[0] == M and b.shape == (N, K)
    elif layout == GEMM_NN:
        K = a.shape[1]
        assert a.shape[0] == M and b.shape == (K, N)
    else:
        K = a.shape[0]
        assert a.shape[1] == M and b.shape == (K, N)
    if residual is not None:
        assert residual.shape == c.shape and residual.stride() == c.stride() and residual.dtype == c.dtype
    if alpha_dev is not None:
        assert alpha_dev.dtype == torch.float32 and alpha_dev.numel() == 1
    check(_lib.load().ssi_gemm(layout, M, N, K, ptr(a), a.stride(0), ptr(b), b.stride(0), ptr(c), c.stride(0),
                               ptr(residual), alpha, ptr(alpha_dev), int(accumulate), dtype_code(c.dtype), stream_ptr()),
          "ssi_gemm")


def splitk_choice(M: int, N: int, K: int, n_cu: int = 256) -> int:
    """Number of K-slices for a 256x256-tiled MFMA GEMM: minimise (waves of workgroups) x (K-tiles per slice) plus the slab
    write + read traffic; 1 when the output grid already fills the chip."""
    if M % 256 or N % 256 or K % 64:
        return 1
    tiles, nk = (M // 256) * (N // 256), K // 64
    if tiles >= 4 * n_cu or tiles % n_cu == 0:
        return 1  # whole rounds, or so many rounds that the partial last one is a small share
    best, best_t = 1, None
    for s in (1, 2, 3, 4, 6, 8, 12, 16):
        if s > nk:
            break
        waves = -(-tiles * s // n_cu)
        t = waves * -(-nk // s) * 1.8e-6 + ((s + 1) * M * N * 4 / 4.0e12 if s > 1 else 0.0)
        if best_t is None or t < best_t * 0.97:
            best, best_t = s, t
    return best


def gemm_splitk(layout: int, a: Tensor, b: Tensor, c: Tensor, splits: int, workspace: Tensor, *, alpha: float = 1.0,
                alpha_dev: Tensor | None = None, accumulate: bool = False, residual: Tensor | None = None) -> None:
    if splits <= 1:
        return gemm(layout, a, b, c, alpha=alpha, alpha_dev=alpha_dev, accumulate=accumulate, residual=residual)
    M, N = c.shape
    K = a.shape[1] if layout in (GEMM_NT, GEMM_NN) else a.shape[0]
    assert a.stride(1) == 1 and b.stride(1) == 1 and c.stride(1) == 1 and a.dtype == b.dtype == c.dtype
    if residual is not None:
        # together with `accumulate` the C entry takes the 8-wave scheme, whose reduction pass adds both (as the unsplit form does)
        assert residual.shape == c.shape and residual.stride() == c.stride() and residual.dtype == c.dtype
    check(_lib.load().ssi_gemm_splitk(layout, M, N, K, ptr(a), a.stride(0), ptr(b), b.stride(0), ptr(c), c.stride(0), ptr(residual),
                                      alpha, ptr(alpha_dev), int(accumulate), dtype_code(c.dtype), splits, ptr(workspace),
                                      workspace.numel() * workspace.element_size(), stream_ptr()), "ssi_gemm_splitk")


def gemm_batched(layout: int, a: Tensor, b: Tensor, c: Tensor, *, alpha: float = 1.0, alpha_dev: Tensor | None = None,
                 accumulate: bool = False) -> None:
    """c[i] = (accumulate ? c[i] : 0) + alpha * op(a[i]) op(b[i]) for every i of the leading dimension, ONE launch on the MFMA path.
    3-D operands with unit inner stride; the leading (batch) stride is free, so ``c`` may be a strided view of the flat gradient."""
    assert a.dim() == 3 and b.dim() == 3 and c.dim() == 3 and a.shape[0] == b.shape[0] == c.shape[0]
    assert a.stride(2) == 1 and b.stride(2) == 1 and c.stride(2) == 1 and a.dtype == b.dtype == c.dtype
    n, M, N = c.shape
    if layout == GEMM_NT:
        K = a.shape[2]
        assert a.shape[1] == M and b.shape[1:] == (N, K)
    elif layout == GEMM_NN:
        K = a.shape[2]
        assert a.shape[1] == M and b.shape[1:] == (K, N)
    else:
        K = a.shape[1]
        assert a.shape[2] == M and b.shape[1:] == (K, N)
    if alpha_dev is not None:
        assert alpha_dev.dtype == torch.float32 and alpha_dev.numel() == 1
    check(_lib.load().ssi_gemm_batched(layout, n, M, N, K, ptr(a), a.stride(1), a.stride(0), ptr(b), b.stride(1), b.stride(0), ptr(c),
                                       c.stride(1), c.stride(0), alpha, ptr(alpha_dev), int(accumulate), dtype_code(c.dtype), stream_ptr()),
          "ssi_gemm_batched")


def gemm_swiglu_fwd(x: Tensor, w13: Tensor, gu: Tensor, act: Tensor) -> None:
    """gu = x @ w13^T ([gate | up]); act = silu(gate) * up — one launch on the MFMA path."""
    M, K = x.shape
    inter = act.shape[1]
    assert w13.shape == (2 * inter, K) and gu.shape == (M, 2 * inter) and act.shape[0] == M
    assert x.stride(1) == 1 and w13.stride(1) == 1 and gu.is_contiguous() and act.is_contiguous()
    check(_lib.load().ssi_gemm_swiglu_fwd(M, inter, K, ptr(x), x.stride(0), ptr(w13), w13.stride(0), ptr(gu), gu.stride(0), ptr(act),
                                          act.stride(0), dtype_code(x.dtype), stream_ptr()), "ssi_gemm_swiglu_fwd")


def gemm_swiglu_bwd(layout: int, dy: Tensor, w2: Tensor, gu: Tensor, dgu: Tensor, dact_ws: Tensor | None) -> None:
    """dgu = swiglu_backward(dy @ W2, gu); w2 is [I, K] for GEMM_NT (transposed copy) or [K, I] for GEMM_NN."""
    M, K = dy.shape
    inter = gu.shape[1] // 2
    assert w2.shape == ((inter, K) if layout == GEMM_NT else (K, inter)) and dgu.shape == gu.shape and gu.shape[0] == M
    assert dy.stride(1) == 1 and w2.stride(1) == 1 and gu.is_contiguous() and dgu.is_contiguous()
    check(_lib.load().ssi_gemm_swiglu_bwd(layout, M, inter, K, ptr(dy), dy.stride(0), ptr(w2), w2.stride(0), ptr(gu), gu.stride(0),
                                          ptr(dgu), dgu.stride(0), ptr(dact_ws), dtype_code(dy.dtype), stream_ptr()),
          "ssi_gemm_swiglu_bwd")


def _w8_rows(codes: Tensor, exps: Tensor, like: Tensor) -> tuple[int, int]:
    """(N, K) of a quantised weight matrix as the ``_w8`` entries take it: uint8 ``codes`` [N, K] (rows may be pitched) and ``exps`` [N]."""
    assert codes.dim() == 2 and codes.dtype == torch.uint8 and codes.stride(1) == 1 and like.dtype == torch.bfloat16
    assert exps.dtype == torch.uint8 and exps.shape == (codes.shape[0],) and exps.is_contiguous() and exps.device == codes.device == like.device
    return codes.shape


def _skinny_weight(w: Tensor, exps: Tensor | None, like: Tensor) -> tuple[int, int]:
    """(N, K) of a skinny GEMM's weight matrix: bf16 ``w`` [N, K] of ``like``'s dtype, or, with ``exps``, the codes of ``_w8_rows``."""
    if exps is not None:
        return _w8_rows(w, exps, like)
    assert w.dim() == 2 and w.stride(1) == 1 and w.dtype == like.dtype
    return w.shape


def _skinny_shapes(a: Tensor, w: Tensor, exps: Tensor | None, c: Tensor, *, residual: Tensor | None = None, rope: tuple | None = None) -> tuple[int, int, int]:
    """(M, N, K) of ``c = a @ w^T`` on a skinny entry, plain (``exps`` None) or ``_w8``: what the plain and the RoPE wrappers ask of ``a``, the weights,
    ``c``, the residual and ``rope`` = (table, positions, head_dim)."""
    assert a.dim() == 2 and c.dim() == 2 and a.stride(1) == 1 and c.stride(1) == 1
    M, K = a.shape
    N, wk = _skinny_weight(w, exps, a)
    assert wk == K and c.shape == (M, N) and a.dtype == c.dtype
    if residual is not None:
        assert residual.shape == c.shape and residual.stride() == c.stride() and residual.dtype == c.dtype
    if rope is not None:
        table, positions, head_dim = rope
        assert table.dtype == torch.float32 and table.is_contiguous() and table.shape[1] * 2 == head_dim
        assert positions.dtype == torch.int32 and positions.numel() == M and positions.is_contiguous()
    return M, N, K


def _skinny_swiglu_shapes(x: Tensor, w13: Tensor, exps13: Tensor | None, gu: Tensor | None, act: Tensor) -> tuple[int, int, int]:
    """(M, I, K) of the SwiGLU form, plain or ``_w8``: ``w13`` = [gate rows | up rows] is [2 I, K], ``act`` [M, I], ``gu`` None or [M, 2 I]."""
    M, K = x.shape
    inter = act.shape[1]
    assert _skinny_weight(w13, exps13, x) == (2 * inter, K) and act.shape[0] == M and x.stride(1) == 1 and act.stride(1) == 1
    assert gu is None or (gu.shape == (M, 2 * inter) and gu.stride(1) == 1 and gu.dtype == x.dtype)
    assert x.dtype == act.dtype
    return M, inter, K


def gemm_skinny(a: Tensor, w: Tensor, c: Tensor, *, residual: Tensor | None = None) -> None:
    """c = a @ w^T (+ residual) for 1 to 64 rows of bf16: the weight-streaming kernel of small-batch decoding (``ssi_gemm``'s rounding points)."""
    M, N, K = _skinny_shapes(a, w, None, c, residual=residual)
    check(_lib.load().ssi_gemm_skinny(M, N, K, ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(c), c.stride(0), ptr(residual),
                                      dtype_code(c.dtype), stream_ptr()), "ssi_gemm_skinny")


def gemm_skinny_rope(a: Tensor, w: Tensor, c: Tensor, n_heads_rot: int, head_dim: int, table: Tensor, positions: Tensor) -> None:
    """``gemm_skinny`` followed by ``rope_`` on the first ``n_heads_rot`` heads of every row, by ``positions`` (required), in one launch."""
    M, N, K = _skinny_shapes(a, w, None, c, rope=(table, positions, head_dim))
    check(_lib.load().ssi_gemm_skinny_rope(M, N, K, ptr(a), a.stride(0), ptr(w), w.stride(0), ptr(c), c.stride(0), n_heads_rot, head_dim,
                                           ptr(table), table.shape[0], ptr(positions), dtype_code(a.dtype), stream_ptr()), "ssi_gemm_skinny_rope")


def gemm_skinny_swiglu(x: Tensor, w13: Tensor, gu: Tensor | None, act: Tensor) -> None:
    """act = silu(gate) * up of ``x @ w13^T`` = [gate | up] for 1 to 64 rows, one launch; ``gu`` (``None``: not written) gets [gate | up]."""
    M, inter, K = _skinny_swiglu_shapes(x, w13, None, gu, act)
    check(_lib.load().ssi_gemm_skinny_swiglu(M, inter, K, ptr(x), x.stride(0), ptr(w13), w13.stride(0), ptr(gu), 0 if gu is None else gu.stride(0),
                                             ptr(act), act.stride(0), dtype_code(x.dtype), stream_ptr()), "ssi_gemm_skinny_swiglu")


def weight_quant_fp8(w: Tensor, codes: Tensor, exps: Tensor) -> None:
    """bf16 ``w`` [N, K] -> e4m3 ``codes`` (uint8 [N, K], rows may be pitched) and one exponent byte per row in ``exps`` (uint8 [N]): the header's
    "FP8 weights" (the "FP8 K/V cache" rule with a row of ``w`` as the line)."""
    assert w.dim() == 2 and w.stride(1) == 1
    N, K = _w8_rows(codes, exps, w)
    assert w.shape == (N, K)
    check(_lib.load().ssi_weight_quant_fp8(ptr(w), w.stride(0), N, K, ptr(codes), codes.stride(0), ptr(exps), dtype_code(w.dtype), stream_ptr()),
          "ssi_weight_quant_fp8")


def gemm_skinny_w8(a: Tensor, codes: Tensor, exps: Tensor, c: Tensor, *, residual: Tensor | None = None) -> None:
    """``gemm_skinny`` on a weight matrix quantised by ``weight_quant_fp8``: bit-equal to ``gemm_skinny`` on the dequantised matrix in bf16."""
    M, N, K = _skinny_shapes(a, codes, exps, c, residual=residual)
    check(_lib.load().ssi_gemm_skinny_w8(M, N, K, ptr(a), a.stride(0), ptr(codes), codes.stride(0), ptr(exps), ptr(c), c.stride(0), ptr(residual),
                                         dtype_code(c.dtype), stream_ptr()), "ssi_gemm_skinny_w8")


def gemm_skinny_rope_w8(a: Tensor, codes: Tensor, exps: Tensor, c: Tensor, n_heads_rot: int, head_dim: int, table: Tensor, positions: Tensor) -> None:
    """``gemm_skinny_rope`` on a quantised weight matrix."""
    M, N, K = _skinny_shapes(a, codes, exps, c, rope=(table, positions, head_dim))
    check(_lib.load().ssi_gemm_skinny_rope_w8(M, N, K, ptr(a), a.stride(0), ptr(codes), codes.stride(0), ptr(exps), ptr(c), c.stride(0), n_heads_rot,
                                              head_dim, ptr(table), table.shape[0], ptr(positions), dtype_code(a.dtype), stream_ptr()),
          "ssi_gemm_skinny_rope_w8")


def gemm_skinny_swiglu_w8(x: Tensor, codes13: Tensor, exps13: Tensor, gu: Tensor | None, act: Tensor) -> None:
    """``gemm_skinny_swiglu`` on a quantised ``w13`` = [gate rows | up rows]."""
    M, inter, K = _skinny_swiglu_shapes(x, codes13, exps13, gu, act)
    check(_lib.load().ssi_gemm_skinny_swiglu_w8(M, inter, K, ptr(x), x.stride(0), ptr(codes13), codes13.stride(0), ptr(exps13), ptr(gu),
                                                0 if gu is None else gu.stride(0), ptr(act), act.stride(0), dtype_code(x.dtype), stream_ptr()),
          "ssi_gemm_skinny_swiglu_w8")


def transpose(src: Tensor, dst: Tensor) -> None:
    """dst[c, r] = src[r, c] (2-D, unit inner stride, dims multiples of 8)."""
    assert src.dim() == 2 and dst.dim() == 2 and src.stride(1) == 1 and dst.stride(1) == 1 and src.dtype == dst.dtype
    assert dst.shape == (src.shape[1], src.shape[0])
    check(_lib.load().ssi_transpose(ptr(src), src.stride(0), ptr(dst), dst.stride(0), src.shape[0], src.shape[1],
                                    dtype_code(src.dtype), stream_ptr()), "ssi_transpose")


def _row_buf_ok(t: Tensor, rows: int, dtype: torch.dtype = torch.float32) -> bool:
    return t.dtype == dtype and t.is_contiguous() and t.numel() >= rows


def _ce_rows(logits: Tensor, labels: Tensor, row_loss: Tensor, row_lse: Tensor | None, row_weight: Tensor | None) -> int:
    """What the ``ce_fwd*`` wrappers ask of the arguments they share; the row count."""
    assert logits.dim() == 2 and logits.stride(1) == 1 and labels.dtype == torch.int64 and labels.is_contiguous()
    rows = logits.shape[0]
    assert labels.numel() == rows and _row_buf_ok(row_loss, rows) and (row_lse is None or _row_buf_ok(row_lse, rows))
    assert row_weight is None or (_row_buf_ok(row_weight, rows) and row_weight.numel() == rows and row_weight.device == logits.device)
    return rows


def ce_fwd(logits: Tensor, labels: Tensor, vocab: int, ignore_index: int, row_loss: Tensor, row_lse: Tensor | None,
           write_grad: bool, row_weight: Tensor | None = None) -> None:
    """``row_weight`` (fp32, one per row, >= 0; ``ssi_ce_fwd_weighted``): loss and gradient of row r times ``row_weight[r]``."""
    rows = _ce_rows(logits, labels, row_loss, row_lse, row_weight)
    if row_weight is None:
        check(_lib.load().ssi_ce_fwd(ptr(logits), logits.stride(0), ptr(labels), rows, vocab, ignore_index, ptr(row_loss),
                                     ptr(row_lse), int(write_grad), dtype_code(logits.dtype), stream_ptr()), "ssi_ce_fwd")
        return
    check(_lib.load().ssi_ce_fwd_weighted(ptr(logits), logits.stride(0), ptr(labels), ptr(row_weight), rows, vocab, ignore_index, ptr(row_loss),
                                          ptr(row_lse), int(write_grad), dtype_code(logits.dtype), stream_ptr()), "ssi_ce_fwd_weighted")


def ce_fwd_z(logits: Tensor, labels: Tensor, vocab: int, ignore_index: int, z_coeff: float, row_loss: Tensor, row_lse: Tensor | None,
             row_z: Tensor, write_grad: bool, row_weight: Tensor | None = None) -> None:
    """``ce_fwd`` with the auxiliary z-loss ``z_coeff * log^2 Z`` in the gradient (``ssi_ce_fwd_z``): ``row_loss`` and ``row_lse`` are those of
    ``ce_fwd`` bit for bit, ``row_z[r] = w_r lse_r^2`` (fp32, the coefficient NOT applied; 0 for an ignored or out-of-range label), and the
    gradient row is ``w (f softmax - onehot)`` with ``f = 1 + 2 z_coeff lse``.  ``z_coeff == 0``: the gradient of ``ce_fwd`` bit for bit."""
    rows = _ce_rows(logits, labels, row_loss, row_lse, row_weight)
    assert _row_buf_ok(row_z, rows)
    check(_lib.load().ssi_ce_fwd_z(ptr(logits), logits.stride(0), ptr(labels), ptr(row_weight), rows, vocab, ignore_index, float(z_coeff),
                                   ptr(row_loss), ptr(row_lse), ptr(row_z), int(write_grad), dtype_code(logits.dtype), stream_ptr()), "ssi_ce_fwd_z")


def ce_fwd_smooth(logits: Tensor, labels: Tensor, vocab: int, ignore_index: int, smoothing: float, z_coeff: float, row_loss: Tensor,
                  row_lse: Tensor | None, row_u: Tensor, row_z: Tensor | None, write_grad: bool, row_weight: Tensor | None = None) -> None:
    """``ce_fwd_z`` with label smoothing ``e = smoothing`` in ``[0, 1)`` (``ssi_ce_fwd_smooth``): ``row_loss``, ``row_lse`` and ``row_z`` are those
    of ``ce_fwd_z`` bit for bit (``row_z`` may be ``None`` when ``z_coeff == 0``), ``row_u[r] = w_r (lse_r - mean_c x[r, c])`` (fp32, the
    coefficient NOT applied; 0 for an ignored or out-of-range label), and the gradient row is
    ``w (f softmax - (1 - e) onehot) - w e / vocab`` on the real columns.  ``smoothing == 0``: the gradient of ``ce_fwd_z`` bit for bit."""
    rows = _ce_rows(logits, labels, row_loss, row_lse, row_weight)
    assert _row_buf_ok(row_u, rows) and (row_z is None or _row_buf_ok(row_z, rows))
    check(_lib.load().ssi_ce_fwd_smooth(ptr(logits), logits.stride(0), ptr(labels), ptr(row_weight), rows, vocab, ignore_index, float(smoothing),
                                        float(z_coeff), ptr(row_loss), ptr(row_lse), ptr(row_u), ptr(row_z), int(write_grad),
                                        dtype_code(logits.dtype), stream_ptr()), "ssi_ce_fwd_smooth")


def ce_fwd_kl(logits: Tensor, teacher: Tensor, teacher_lse: Tensor, labels: Tensor, vocab: int, ignore_index: int, kl_coeff: float,
              row_loss: Tensor, row_lse: Tensor | None, row_kl: Tensor, write_grad: bool, row_weight: Tensor | None = None,
              row_kl_weight: Tensor | None = None) -> None:
    """``ce_fwd`` with ``kl_coeff * KL(teacher || student)`` in the gradient (``ssi_ce_fwd_kl``).  ``teacher`` holds a frozen model's logits on the
    same rows (same dtype and device, its own row stride; read only) and ``teacher_lse`` what ``ce_fwd(teacher, ..., write_grad=False)`` wrote as
    ``row_lse`` with the same labels.  ``row_loss`` and ``row_lse`` are those of ``ce_fwd`` bit for bit, ``row_kl[r] = k_r KL(q_r || p_r)`` (fp32,
    the coefficient NOT applied; 0 for an ignored or out-of-range label) with ``k = row_kl_weight`` (``None``: the row's ``row_weight``), and the
    gradient row is ``(w + b k) softmax - w onehot - b k q``.  ``kl_coeff == 0``: the gradient of ``ce_fwd`` bit for bit."""
    rows = _ce_rows(logits, labels, row_loss, row_lse, row_weight)
    assert teacher.dim() == 2 and teacher.stride(1) == 1 and teacher.shape == logits.shape and teacher.dtype == logits.dtype
    assert teacher.device == logits.device and _row_buf_ok(teacher_lse, rows) and _row_buf_ok(row_kl, rows)
    assert row_kl_weight is None or (_row_buf_ok(row_kl_weight, rows) and row_kl_weight.numel() == rows and row_kl_weight.device == logits.device)
    check(_lib.load().ssi_ce_fwd_kl(ptr(logits), logits.stride(0), ptr(teacher), teacher.stride(0), ptr(teacher_lse), ptr(labels), ptr(row_weight),
                                    ptr(row_kl_weight), rows, vocab, ignore_index, float(kl_coeff), ptr(row_loss), ptr(row_lse), ptr(row_kl),
                                    int(write_grad), dtype_code(logits.dtype), stream_ptr()), "ssi_ce_fwd_kl")


def ce_reduce(row_loss: Tensor, labels: Tensor, vocab: int, ignore_index: int, out: Tensor) -> None:
    """out[0] mean NLL over valid labels, out[1] sum, out[2] valid count, out[3] labels that are neither ignored nor in [0, vocab)."""
    assert out.dtype == torch.float32 and out.numel() >= 4 and labels.is_contiguous()
    check(_lib.load().ssi_ce_reduce(ptr(row_loss), ptr(labels), labels.numel(), vocab, ignore_index, ptr(out), stream_ptr()),
          "ssi_ce_reduce")


def ce_fwd_metrics(logits: Tensor, labels: Tensor, vocab: int, ignore_index: int, row_loss: Tensor, row_lse: Tensor | None, row_nll: Tensor,
                   row_rank: Tensor, row_weight: Tensor | None = None) -> None:
    """Forward-only ``ce_fwd`` (``write_grad=False``; ``row_loss`` and ``row_lse`` bit for bit) that also writes the unweighted ``row_nll`` (fp32)
    and ``row_rank`` (int32): the label's position in a stable descending sort of its row, -1 for an ignored or out-of-range label."""
    rows = _ce_rows(logits, labels, row_loss, row_lse, row_weight)
    assert _row_buf_ok(row_nll, rows) and _row_buf_ok(row_rank, rows, torch.int32)
    check(_lib.load().ssi_ce_fwd_metrics(ptr(logits), logits.stride(0), ptr(labels), ptr(row_weight), rows, vocab, ignore_index, ptr(row_loss),
                                         ptr(row_lse), ptr(row_nll), ptr(row_rank), dtype_code(logits.dtype), stream_ptr()), "ssi_ce_fwd_metrics")


def ce_metrics_reduce(row_nll: Tensor, row_rank: Tensor, labels: Tensor, ranges: Tensor, topk: int, out: Tensor, accumulate: bool = False) -> None:
    """``out`` (fp64 ``[n_ranges + 1, 4]``) = per label range, and last for every valid label: n_labels, sum nll, n(rank == 0), n(rank < topk).
    ``ranges``: int64 inclusive ``[lo, hi]`` pairs as for ``count_tokens``.  ``accumulate``: add to what ``out`` holds."""
    n_ranges, rows = ranges.numel() // 2, labels.numel()
    assert row_nll.dtype == torch.float32 and row_nll.is_contiguous() and row_nll.numel() >= rows
    assert row_rank.dtype == torch.int32 and row_rank.is_contiguous() and row_rank.numel() >= rows
    assert labels.dtype == torch.int64 and labels.is_contiguous() and ranges.dtype == torch.int64 and ranges.is_contiguous()
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= 4 * (n_ranges + 1) and topk >= 1
    check(_lib.load().ssi_ce_metrics_reduce(ptr(row_nll), ptr(row_rank), ptr(labels), rows, ptr(ranges), n_ranges, int(topk), int(accumulate),
                                            ptr(out), stream_ptr()), "ssi_ce_metrics_reduce")


def seq_score_reduce(row_nll: Tensor, row_rank: Tensor, rows: int, seq_start: Tensor, seq_end: Tensor, topk: int, out: Tensor) -> None:
    """``out`` (fp64 ``[n_seq, 4]``, overwritten) = per sequence n_labels, sum nll, n(rank == 0), n(rank < topk) over the flat positions
    ``[seq_start[i], seq_end[i])`` (int64 device tensors; clamped to ``[0, rows]``) of what ``ce_fwd_metrics`` wrote."""
    n_seq = seq_start.numel()
    assert row_nll.dtype == torch.float32 and row_nll.is_contiguous() and row_nll.numel() >= rows
    assert row_rank.dtype == torch.int32 and row_rank.is_contiguous() and row_rank.numel() >= rows
    assert seq_start.dtype == torch.int64 and seq_start.is_contiguous() and seq_end.dtype == torch.int64 and seq_end.is_contiguous()
    assert seq_end.numel() == n_seq and out.dtype == torch.float64 and out.is_contiguous() and out.numel() >= 4 * n_seq
    check(_lib.load().ssi_seq_score_reduce(ptr(row_nll), ptr(row_rank), int(rows), ptr(seq_start), ptr(seq_end), n_seq, int(topk), ptr(out),
                                           stream_ptr()), "ssi_seq_score_reduce")


def edit_distance(tokens: Tensor, ref_start: Tensor, ref_len: Tensor, hyp_start: Tensor, hyp_len: Tensor, out: Tensor, max_len: int) -> None:
    """``out`` (int32 ``[n_pairs, 4]``, overwritten) = ``{dist, S, D, I}`` of the edit distance between the spans
    ``tokens[ref_start[p] : + ref_len[p]]`` and ``tokens[hyp_start[p] : + hyp_len[p]]`` of one flat int32 device buffer (starts int64, lengths
    int32, device tensors the host never reads).  ``max_len`` (at most ``_lib.EDIT_MAX_LEN``) bounds every length; a pair with a span that is
    longer, negative or outside ``tokens`` gets four -1.  The definition is in ``include/ssi_hip.h``."""
    lib = _lib.load()
    n_pairs = ref_start.numel()
    assert tokens.dtype == torch.int32 and tokens.is_contiguous() and out.dtype == torch.int32 and out.is_contiguous() and out.numel() >= 4 * n_pairs
    for start, length in ((ref_start, ref_len), (hyp_start, hyp_len)):
        assert start.dtype == torch.int64 and start.is_contiguous() and length.dtype == torch.int32 and length.is_contiguous()
        assert start.numel() == n_pairs and length.numel() == n_pairs
    need = lib.ssi_edit_distance_workspace_bytes(n_pairs, int(max_len))
    workspace = _byte_ws(need, tokens) if need else None
    check(lib.ssi_edit_distance(ptr(tokens), tokens.numel(), ptr(ref_start), ptr(ref_len), ptr(hyp_start), ptr(hyp_len), n_pairs, int(max_len),
                                ptr(out), ptr(workspace), need, stream_ptr()), "ssi_edit_distance")


def _bpe_i32(*tensors: Tensor) -> None:
    for t in tensors:
        assert t.dtype == torch.int32 and t.is_contiguous(), "unit BPE buffers are contiguous int32 device tensors"


def bpe_pair_count(ids: Tensor, V: int, stride: int, table: Tensor, n_bad: Tensor | None = None) -> None:
    """``table[a * stride + b] += c(a, b)`` over the flat int32 buffer ``ids`` (separator -1; ``table`` int32 of at least ``V * stride`` entries,
    cleared by the caller).  An id outside ``[0, V)`` other than -1 acts as a separator and is counted once into ``n_bad`` (int32 ``[1]``, added
    to).  The definition is in ``include/ssi_hip.h``."""
    _bpe_i32(ids, table, *([n_bad] if n_bad is not None else []))
    assert 0 < V <= stride and table.numel() >= (V - 1) * stride + V
    check(_lib.load().ssi_bpe_pair_count(ptr(ids), ids.numel(), int(V), int(stride), ptr(table), ptr(n_bad), stream_ptr()), "ssi_bpe_pair_count")


def bpe_train_workspace_bytes(n: int) -> int:
    return int(_lib.load().ssi_bpe_train_workspace_bytes(int(n)))


def bpe_train_begin(ids: Tensor, n_base: int, v_cap: int, buf0: Tensor, table: Tensor, state: Tensor) -> None:
    """Start a training: ``table`` (int32 ``[v_cap * v_cap]``) cleared and filled with the pair counts of ``ids``, ``buf0`` = ``ids`` with bad ids
    replaced by -1, ``state`` (int32 ``[_lib.BPE_STATE_WORDS]``) set: length of buffer 0, ``n_bad``, everything else zero."""
    _bpe_i32(ids, buf0, table, state)
    assert buf0.numel() >= ids.numel() and table.numel() >= v_cap * v_cap and state.numel() >= _lib.BPE_STATE_WORDS
    check(_lib.load().ssi_bpe_train_begin(ptr(ids), ids.numel(), int(n_base), int(v_cap), ptr(buf0), ptr(table), ptr(state), stream_ptr()),
          "ssi_bpe_train_begin")


def bpe_merge(buf0: Tensor, buf1: Tensor, n_upper: int, n_base: int, v_cap: int, m: int, min_frequency: int, table: Tensor, merges: Tensor,
              state: Tensor, workspace: Tensor) -> None:
    """Launch merge ``m`` (it reads buffer ``m & 1`` and writes the other; the pair, the lengths and ``done`` are read from ``state`` on the
    device, and after ``done`` the launches do nothing).  ``n_upper``: the host's bound on the current length.  Nothing is read back."""
    _bpe_i32(buf0, buf1, table, merges, state)
    assert buf0.numel() == buf1.numel() and table.numel() >= v_cap * v_cap and merges.numel() >= 3 * (v_cap - n_base)
    assert state.numel() >= _lib.BPE_STATE_WORDS and workspace.dtype == torch.uint8
    check(_lib.load().ssi_bpe_merge(ptr(buf0), ptr(buf1), buf0.numel(), int(n_upper), int(n_base), int(v_cap), int(m), int(min_frequency), ptr(table),
                                    ptr(merges), ptr(state), ptr(workspace), workspace.numel(), stream_ptr()), "ssi_bpe_merge")


def bpe_encode(tokens: Tensor, seq_start: Tensor, seq_len: Tensor, max_len: int, rank_table: Tensor, V: int, n_base: int, out: Tensor,
               out_len: Tensor) -> None:
    """Encode the spans ``tokens[seq_start[s] : + seq_len[s]]`` (starts int64, lengths int32) with the merges of ``rank_table`` (int32
    ``[V * V]``, -1: no merge): ``out[seq_start[s] : + out_len[s]]`` holds the result, ``out_len[s]`` is -1 for a bad span.  ``max_len`` (at most
    ``_lib.BPE_ENCODE_MAX_LEN``) bounds every length."""
    _bpe_i32(tokens, seq_len, rank_table, out, out_len)
    n_seq = seq_start.numel()
    assert seq_start.dtype == torch.int64 and seq_start.is_contiguous() and seq_len.numel() == n_seq and out_len.numel() >= n_seq
    assert out.numel() >= tokens.numel() and rank_table.numel() >= V * V
    check(_lib.load().ssi_bpe_encode(ptr(tokens), tokens.numel(), ptr(seq_start), ptr(seq_len), n_seq, int(max_len), ptr(rank_table), int(V), int(n_base),
                                     ptr(out), ptr(out_len), stream_ptr()), "ssi_bpe_encode")


def lmhead_ce_fwd(hidden: Tensor, table: Tensor, labels: Tensor, vocab: int, ignore_index: int, logits_ws: Tensor, row_loss: Tensor,
                  stats: Tensor, write_grad: bool) -> None:
    """Tied LM head + cross-entropy, one ABI call: logits_ws = hidden @ table^T, row losses, stats = (mean, sum, n_valid, n_out_of_range);
    with write_grad logits_ws holds softmax - onehot afterwards."""
    rows, dim = hidden.shape
    vocab_pad = table.shape[0]
    assert table.shape[1] == dim and logits_ws.shape == (rows, vocab_pad) and hidden.stride(1) == 1 and table.stride(1) == 1
    assert labels.dtype == torch.int64 and labels.is_contiguous() and labels.numel() == rows and stats.dtype == torch.float32 and stats.numel() >= 4
    assert row_loss.dtype == torch.float32 and row_loss.numel() >= rows and hidden.dtype == table.dtype == logits_ws.dtype
    check(_lib.load().ssi_lmhead_ce_fwd(ptr(hidden), hidden.stride(0), ptr(table), table.stride(0), ptr(labels), rows, dim, vocab, vocab_pad,
                                        ignore_index, ptr(logits_ws), logits_ws.stride(0), ptr(row_loss), ptr(stats), int(write_grad),
                                        dtype_code(hidden.dtype), stream_ptr()), "ssi_lmhead_ce_fwd")


def lmhead_ce_bwd(dlogits: Tensor, hidden: Tensor, table: Tensor, alpha_dev: Tensor | None, d_hidden: Tensor, d_table: Tensor,
                  accumulate_d_table: bool) -> None:
    """d_hidden = alpha * dlogits @ table;  d_table (+)= alpha * dlogits^T @ hidden."""
    rows, dim = hidden.shape
    vocab_pad = table.shape[0]
    assert dlogits.shape == (rows, vocab_pad) and d_hidden.shape == hidden.shape and d_table.shape == table.shape
    assert alpha_dev is None or (alpha_dev.dtype == torch.float32 and alpha_dev.numel() == 1)
    check(_lib.load().ssi_lmhead_ce_bwd(ptr(dlogits), dlogits.stride(0), ptr(hidden), hidden.stride(0), ptr(table), table.stride(0),
                                        ptr(alpha_dev), rows, dim, vocab_pad, ptr(d_hidden), d_hidden.stride(0), ptr(d_table),
                                        d_table.stride(0), int(accumulate_d_table), dtype_code(hidden.dtype), stream_ptr()), "ssi_lmhead_ce_bwd")


def count_tokens(tokens: Tensor, labels: Tensor | None, ranges: Tensor, pad_id: int, ignore_index: int, out: Tensor) -> None:
    """out[0:n_ranges] range counts, out[n_ranges] non-pad tokens, out[n_ranges+1] non-ignored labels (int64, device)."""
    n_ranges = ranges.numel() // 2
    assert tokens.dtype == torch.int64 and tokens.is_contiguous() and ranges.dtype == torch.int64 and out.dtype == torch.int64
    assert out.numel() >= n_ranges + 2 and (labels is None or (labels.is_contiguous() and labels.numel() == tokens.numel()))
    check(_lib.load().ssi_count_tokens(ptr(tokens), ptr(labels), tokens.numel(), ptr(ranges), n_ranges, pad_id,
                                       ignore_index, ptr(out), stream_ptr()), "ssi_count_tokens")


def scale_(x: Tensor, scale: float = 1.0, scale_dev: Tensor | None = None) -> None:
    assert x.is_contiguous()
    check(_lib.load().ssi_scale_inplace(ptr(x), x.numel(), scale, ptr(scale_dev), dtype_code(x.dtype), stream_ptr()),
          "ssi_scale_inplace")


def sumsq(x: Tensor, out: Tensor, workspace: Tensor | None = None) -> None:
    lib = _lib.load()
    assert x.is_contiguous() and out.dtype == torch.float32
    need = lib.ssi_sumsq_workspace_bytes(x.numel())
    if workspace is None or workspace.numel() * workspace.element_size() < need:
        workspace = _byte_ws(need, x)
    check(lib.ssi_sumsq(ptr(x), x.numel(), dtype_code(x.dtype), ptr(out), ptr(workspace),
                        workspace.numel() * workspace.element_size(), stream_ptr()), "ssi_sumsq")


def sumsq_groups(x: Tensor, seg_end, seg_group, n_groups: int, out: Tensor, workspace: Tensor | None = None) -> None:
    """``out[g]`` = the fp32 sum of squares of the elements of all segments of group ``g`` (``ssi_sumsq_groups``), for every group in one pass
    over ``x``.  Segment ``s`` covers ``[seg_end[s-1], seg_end[s])`` (``adamw_step_seg``'s conventions) and belongs to group ``seg_group[s]`` in
    ``[0, n_groups)``, or, with -1, to none: such a segment is not read.  Both sequences are host values; ``out`` is an fp32 device tensor of
    ``n_groups`` elements, overwritten.  The same inputs give the same bits, and no element outside a group changes its sum."""
    lib = _lib.load()
    n_segs = len(seg_end)
    assert x.is_contiguous() and out.is_contiguous() and out.dtype == torch.float32 and out.numel() == n_groups and len(seg_group) == n_segs >= 1
    need = lib.ssi_sumsq_groups_workspace_bytes(x.numel(), n_segs, n_groups)
    if workspace is None:
        workspace = _byte_ws(need, out)
    ends = (_lib.c_int64 * n_segs)(*[int(e) for e in seg_end])
    groups = (_lib.c_int32 * n_segs)(*[int(g) for g in seg_group])
    check(lib.ssi_sumsq_groups(ptr(x) if x.numel() else None, x.numel(), dtype_code(x.dtype), ends, groups, n_segs, n_groups, ptr(out), ptr(workspace),
                               workspace.numel() * workspace.element_size(), stream_ptr()), "ssi_sumsq_groups")


def _adamw_flags(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, zero_grad: bool, skip_nonfinite_scale: bool) -> int:
    """The AdamW entries' ``zero_grad`` argument, after the checks on the four buffers that they share."""
    assert param.is_contiguous() and grad.is_contiguous() and exp_avg.is_contiguous() and exp_avg_sq.is_contiguous()
    assert param.numel() == grad.numel() == exp_avg.numel() == exp_avg_sq.numel()
    assert param.dtype == grad.dtype == exp_avg.dtype == exp_avg_sq.dtype
    return int(zero_grad) | (2 if skip_nonfinite_scale else 0)


def adamw_step(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, *, lr: float, beta1: float, beta2: float,
               eps: float, weight_decay: float, step: int, grad_scale_dev: Tensor | None = None,
               zero_grad: bool = False, skip_nonfinite_scale: bool = False, sr_seed: int | None = None, elem_offset: int = 0) -> None:
    """``skip_nonfinite_scale``: the launch changes nothing when ``*grad_scale_dev`` is inf or NaN (1 / 0 label tokens: the reference skips such
    a window's optimizer step; an update issued before the host knows the count must do the same by itself).  ``sr_seed`` (bf16 only): the three
    stores round stochastically (``ssi_adamw_step_sr``) with the random bits of ``(sr_seed, step, elem_offset + i, tensor)`` — ``elem_offset``
    is the place of the slice's first element in the whole buffer, a multiple of 8; without a seed it is not used."""
    flags = _adamw_flags(param, grad, exp_avg, exp_avg_sq, zero_grad, skip_nonfinite_scale)
    if sr_seed is not None:
        check(_lib.load().ssi_adamw_step_sr(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), lr, beta1, beta2,
                                            eps, weight_decay, step, ptr(grad_scale_dev), flags, dtype_code(param.dtype),
                                            int(sr_seed) & 0xFFFFFFFFFFFFFFFF, elem_offset, stream_ptr()), "ssi_adamw_step_sr")
        return
    check(_lib.load().ssi_adamw_step(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), lr, beta1, beta2,
                                     eps, weight_decay, step, ptr(grad_scale_dev), flags, dtype_code(param.dtype),
                                     stream_ptr()), "ssi_adamw_step")


def adamw_step_seg(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, *, seg_end, seg_lr, seg_weight_decay, seg_frozen,
                   beta1: float, beta2: float, eps: float, step: int, grad_scale_dev: Tensor | None = None, zero_grad: bool = False,
                   skip_nonfinite_scale: bool = False, sr_seed: int | None = None, elem_offset: int = 0,
                   seg_scale_dev: Tensor | None = None) -> None:
    """``adamw_step`` over consecutive segments of the buffers in one launch (``ssi_adamw_step_seg``): segment ``s`` covers the elements
    ``[seg_end[s-1], seg_end[s])`` (``seg_end[-1] = 0``; ends ascending, multiples of 8 but the last, which is ``numel``) and runs at
    ``seg_lr[s]`` / ``seg_weight_decay[s]``, or is left alone — neither read nor written — where ``seg_frozen[s]``.  The four sequences are
    host values.  More than ``_lib.ADAMW_MAX_SEGS`` segments become several launches, split at segment ends; the result is the same.
    ``seg_scale_dev`` (an fp32 DEVICE tensor of one factor per segment; ``ssi_adamw_step_seg_gscale``): segment ``s`` sees its gradient times
    ``fl(grad_scale_dev * seg_scale_dev[s])`` (``seg_scale_dev[s]`` alone without a ``grad_scale_dev``), and a segment whose factor is inf or
    NaN is left alone like a frozen one.  The split launches take the slices of it that go with their segments."""
    flags = _adamw_flags(param, grad, exp_avg, exp_avg_sq, zero_grad, skip_nonfinite_scale)
    n_segs = len(seg_end)
    assert n_segs >= 1 and len(seg_lr) == len(seg_weight_decay) == len(seg_frozen) == n_segs
    lib, cap = _lib.load(), _lib.ADAMW_MAX_SEGS
    if seg_scale_dev is not None:
        assert seg_scale_dev.dtype == torch.float32 and seg_scale_dev.is_contiguous() and seg_scale_dev.numel() == n_segs
    param, grad, exp_avg, exp_avg_sq = param.view(-1), grad.view(-1), exp_avg.view(-1), exp_avg_sq.view(-1)
    if param.numel() == 0 and n_segs == 1 and int(seg_end[0]) == 0:
        return   # (an empty tensor has no address to hand over)
    for a in range(0, n_segs, cap):
        b = min(a + cap, n_segs)
        lo, hi = (int(seg_end[a - 1]) if a else 0), int(seg_end[b - 1])
        if hi < lo or (a and hi == lo):
            raise ValueError(f"adamw_step_seg: segment ends must ascend (segments {a}..{b})")
        k = b - a
        ends = (_lib.c_int64 * k)(*[int(e) - lo for e in seg_end[a:b]])
        lrs = (_lib.c_double * k)(*[float(x) for x in seg_lr[a:b]])
        wds = (_lib.c_double * k)(*[float(x) for x in seg_weight_decay[a:b]])
        frz = (_lib.c_int32 * k)(*[1 if x else 0 for x in seg_frozen[a:b]])
        sl = slice(lo, hi) if (a or b < n_segs) else slice(None)   # (one launch: the whole buffers, so that a wrong last end is the library's error)
        if seg_scale_dev is not None:
            check(lib.ssi_adamw_step_seg_gscale(ptr(param[sl]), ptr(grad[sl]), ptr(exp_avg[sl]), ptr(exp_avg_sq[sl]), param[sl].numel(), ends, lrs, wds,
                                                frz, k, beta1, beta2, eps, step, ptr(grad_scale_dev), flags, dtype_code(param.dtype),
                                                int(sr_seed is not None), (int(sr_seed) & 0xFFFFFFFFFFFFFFFF) if sr_seed is not None else 0,
                                                elem_offset + lo, ptr(seg_scale_dev[a:b]), stream_ptr()), "ssi_adamw_step_seg_gscale")
            continue
        check(lib.ssi_adamw_step_seg(ptr(param[sl]), ptr(grad[sl]), ptr(exp_avg[sl]), ptr(exp_avg_sq[sl]), param[sl].numel(), ends, lrs, wds, frz, k,
                                     beta1, beta2, eps, step, ptr(grad_scale_dev), flags, dtype_code(param.dtype), int(sr_seed is not None),
                                     (int(sr_seed) & 0xFFFFFFFFFFFFFFFF) if sr_seed is not None else 0, elem_offset + lo, stream_ptr()),
              "ssi_adamw_step_seg")


def round_bf16_sr(src: Tensor, dst: Tensor, *, seed: int, step: int, tensor: int, elem_offset: int = 0) -> None:
    """fp32 -> bf16 by the stochastic rounding of ``adamw_step(sr_seed=...)``: the bits of ``(seed, step, elem_offset + i, tensor)``."""
    assert src.is_contiguous() and dst.is_contiguous() and src.numel() == dst.numel()
    assert src.dtype == torch.float32 and dst.dtype == torch.bfloat16
    check(_lib.load().ssi_round_bf16_sr(ptr(src), ptr(dst), src.numel(), int(seed) & 0xFFFFFFFFFFFFFFFF, step, tensor, elem_offset,
                                        stream_ptr()), "ssi_round_bf16_sr")


def ema_update(ema: Tensor, param: Tensor, *, decay: float, guard_dev: Tensor | None = None) -> None:
    """``ema = fma(decay, ema - param, param)`` per element in fp32 (``ssi_ema_update``): the running average of ``param`` (bf16 or fp32) in the
    fp32 ``ema``.  ``guard_dev``: the launch changes nothing when ``*guard_dev`` is inf or NaN (``adamw_step``'s ``skip_nonfinite_scale``)."""
    if ema.dtype != torch.float32:
        raise TypeError(f"ema_update: the average is kept in fp32, not {ema.dtype}")
    assert ema.is_contiguous() and param.is_contiguous() and ema.numel() == param.numel()
    check(_lib.load().ssi_ema_update(ptr(ema), ptr(param), ema.numel(), float(decay), ptr(guard_dev), dtype_code(param.dtype), stream_ptr()),
          "ssi_ema_update")
